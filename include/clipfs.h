/*
 * clipfs.h -- C ABI of libclipfs_hip.so: the MI355X (gfx950) engine behind the
 * reference's Python API for the CLIP few-shot hot path.
 *
 * The reference (Dokumushikun/jittor-clip-fewshot) has NO FFI / plugin layer:
 * every op below is executed today by Jittor-generated CUDA kernels reached from
 * Python.  Each entry point cites the reference Python site
 * whose arithmetic it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named h_*; tensors are fp32,
 *     row-major, densely packed unless a leading dimension is given;
 *   - activations are token-major: row m = b * L + l  (the reference is
 *     sequence-first [L, N, d]; only the memory order differs, not the values);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - return value: 0 = ok, CLIPFS_EINVAL = bad argument (nothing launched),
 *     otherwise 1000 + hipError_t of the failed launch;
 *   - no entry point allocates or frees device memory or synchronises the stream: all buffers (workspaces
 *     included) are owned by the caller (PyTorch-ROCm tensors).  The only state kept is per host thread:
 *     the last error string and, while enabled, the GEMM timing events (clipfs_gemm_timing).
 */
#ifndef CLIPFS_H
#define CLIPFS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIPFS_OK 0
#define CLIPFS_EINVAL 1
#define CLIPFS_HIPERR_BASE 1000

/* Version 2 (round 3): the descriptor structs (clipfs_gemm_args, clipfs_tower) start with `struct_size` = sizeof of the
 * struct the CALLER was compiled against; the library rejects (CLIPFS_EINVAL, nothing launched) a size it does not know
 * instead of reading fields at shifted offsets.  New fields are appended at the END of a struct only; a change that moves
 * an existing field or a parameter of an entry point bumps this number.  Version 1 (rounds 1-2) had no size member and
 * changed layout once without a bump: binaries built against it must be rebuilt. */
#define CLIPFS_ABI_VERSION 2
int clipfs_abi_version(void);
/* sha256 prefixes (16 hex digits) of the sources the library was built from: all of csrc/ + this header, and the
 * fp32 GEMM alone (gemm.hip, gemm_common.h, common.h).  "unstamped" when built without build.py. */
const char* clipfs_source_stamp(void);
const char* clipfs_gemm_source_stamp(void);
/* human readable description of the last CLIPFS_EINVAL on this thread */
const char* clipfs_last_error(void);

/* ------------------------------------------------------------------ GEMM --
 * C[M,N] = epilogue( alpha * A[M,K] * B[N,K]^T )      fp32 MFMA (v_mfma_f32_32x32x2_f32)
 * Replaces every jittor.nn.linear / matmul on the path: packed QKV (jclip/mha.py:140),
 * LinearLoRA (lora_train_vlp.py:286-306), out_proj (mha.py:461), MLP (jclip/model.py:34-39),
 * patch-embed conv (model.py:87-91,105), visual.proj / text_projection (model.py:124,213-214),
 * cosine logits (lora_train_vlp.py:995), and their input-gradients.
 * Epilogue, in this order (each part optional):
 *     v  = alpha * acc + bias[n]
 *     v += lora_scale * sum_j lora_t[m, seg*r + j] * lora_b[n, j]      seg = n / lora_seg_width
 *         (the f16 x f16 kernel adds this product inside its accumulator, i.e. before alpha: it refuses lora_t with
 *          alpha != 1 -- CLIPFS_EINVAL -- rather than scale the adapter term; no caller combines the two)
 *     if act == 1:  (aux_out[m,n] = v);  v = v * sigmoid(1.702 v)        QuickGELU, model.py:24-27
 *     if act == 2:  v = v * dQuickGELU(aux_in[m,n])                      backward of act 1
 *     v += residual[rm, n]                                               model.py:60-61
 *     if act == 3:  v = max(v, 0)                                        ReLU after the residual add (the ResNet-50
 *                                                                        bottleneck of the MoCo branch, slow_pace.py:1239)
 *     C[out_row(m), n] = v
 * a_mode 0: A is row-major [M,K] with leading dimension lda.
 * a_mode 1: A is an NCHW image batch [B,3,R,R]; row m = (b, py, px) patch, column
 *           k = (c, ky, kx)  (im2col on the fly, kernel = stride = patch).  Then
 *           out_row(m) = b*out_tokens + 1 + p and residual row rm = 1 + p  (p = m % P):
 *           class-token slot skipped, positional embedding added (model.py:105-114).
 */
typedef struct clipfs_gemm_args {
  size_t struct_size;      /* = sizeof(clipfs_gemm_args) of the caller's header (ABI check) */
  const float* A;
  const float* B;          /* [N,K] row-major, ldb */
  float* C;                /* [*,N] row-major, ldc */
  int M, N, K;
  int lda, ldb, ldc;
  float alpha;
  const float* bias;       /* [N] or NULL */
  const float* residual;   /* [*,N] (ld = ldres) or NULL */
  int ldres;
  int act;                 /* 0 none, 1 QuickGELU, 2 multiply by dQuickGELU(aux_in), 3 ReLU (after the residual; fp32 only) */
  float* aux_out;          /* act 1: pre-activation copy (ld = ldc) or NULL */
  const float* aux_in;     /* act 2: saved pre-activation (ld = ldc) */
  const float* lora_t;     /* [M, lora_nseg * lora_r] or NULL */
  const float* lora_b;     /* [N, lora_r] */
  int lora_r, lora_nseg, lora_seg_width; /* f16 x f16 kernel: lora_r <= 64, lora_seg_width % 128 == 0 */
  float lora_scale;
  int a_mode;              /* 0 dense, 1 patch im2col */
  int img_res, patch, out_tokens; /* a_mode 1 */
  const void* B_planes;    /* optional 16-bit copy of B (a_mode 0, K % 32 == 0, ldb == K); NULL = exact fp32 */
  int b_format;            /* 1: bf16 hi/lo planes (clipfs_split_bf16) -> split-bf16 x3 kernel;
                              2: one f16 plane (clipfs_convert_f16) -> f16 MFMA kernel (cfg-5's fp16 path) */
  float* workspace;        /* optional split-K slab scratch, 16-byte aligned (NULL: never split) */
  size_t workspace_floats;
  const void* A_f16;       /* optional f16 copy of A [M,K] (ld = lda): with b_format 2 selects the f16 x f16 kernel
                              (operands stream HBM -> LDS -> MFMA untouched); A may then be NULL */
  void* C_f16;             /* f16 x f16 kernel only: also (or, with C == NULL, only) write the result as f16, ld = ldc */
  int aux_f16;             /* f16 x f16 kernel only: aux_out / aux_in hold f16 values (fp16 storage of the saved
                              pre-activation), ld = ldc */
  int* counters;           /* optional arrival counters (split-K): >= clipfs_gemm_counter_ints(M,N,K) ints, ZERO on
                              entry (the kernel leaves them zero); with `workspace` enables the split */
  size_t counters_ints;
} clipfs_gemm_args;
/* Ordering: everything the call does is ordered on `stream` (work queued on it before the call happens-before, work
 * queued after it happens-after).  The f16 x f16 path may run part of the rows on an internal high-priority side
 * stream, forked from and joined back into `stream` with events inside the call (one side stream per caller stream
 * and host thread, created on first use). */
int clipfs_gemm_nt(const clipfs_gemm_args* args, void* stream);
/* Products with few output tiles (small per-rank batches, the one-row-per-sequence products of the last block) are
 * cut along K into `clipfs_gemm_splits` slices.  Every slice writes its raw partial tile to `workspace` and the slice
 * that arrives LAST at the tile's arrival counter (`counters`) adds the slices in slice order and applies the epilogue,
 * inside the same launch -- deterministic, no float atomics, no second kernel.  Enabled when workspace_floats >=
 * clipfs_gemm_workspace_floats(M,N,K) AND counters_ints >= clipfs_gemm_counter_ints(M,N,K) (both 0 for shapes that
 * are never split); `counters` must be zero on entry and is left zero. */
/* planes[0..n) = bf16(src), planes[n..2n) = bf16(src - hi): the frozen-weight half of the opt-in split-bf16
 * ("bf16 x 3") GEMM: a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_32x32x16_bf16, fp32 accumulate.
 * `planes` holds 2*n bf16 values (4*n bytes); n % 8 == 0. */
int clipfs_split_bf16(const float* src, void* planes, size_t n, void* stream);
/* dst[0..n) = f16(src): weights for the fp16 MFMA mode (v_mfma_f32_32x32x16_f16, fp32 accumulate; activations are
 * rounded to f16 in the staging path).  Tolerance is that of fp16 products (~5e-4 relative), stated in the tests. */
int clipfs_convert_f16(const float* src, void* dst, size_t n, void* stream);
/* The dispatch of the exact fp32 and the 16-bit-plane kernels as data: clipfs_gemm_plan IS the function clipfs_gemm_nt
 * executes (validate, plan, one switch over `kernel`).  Host-only: nothing is launched and no pointer of `args` is
 * dereferenced; their nullness and 16-byte alignment take part in the choice.  Returns CLIPFS_EINVAL with the refusal's
 * message for arguments clipfs_gemm_nt would refuse (`plan` is left untouched), and with A_f16 set: that kernel's plan
 * is clipfs_gemm_f16_plan.  The schedule is stated for the MI355X's 256 CUs.  The aids CLIPFS_GEMM_BM (32 / 64),
 * _SPLITS, _GM, _LDS_PAD (KiB), _GLDS=0 and CLIPFS_BF16_TILE (1 / 2) are read once per process and show in the plan. */
#define CLIPFS_GEMM_NT64 0       /* dense, K % 32 == 0: 64 x 128 tile, operands staged by LDS-DMA */
#define CLIPFS_GEMM_NT64_REG 1   /*   the same staged through registers (CLIPFS_GEMM_GLDS=0) */
#define CLIPFS_GEMM_NT32 2       /*   32 x 128 tile */
#define CLIPFS_GEMM_MIXED 3      /*   rows [0, mix_rows64) as 64 x 128 tiles, the rows behind them as 32 x 128, one launch */
#define CLIPFS_GEMM_PATCH32 4    /* a_mode 1 with patch 32 and 16-byte aligned image rows: 64 x 128 */
#define CLIPFS_GEMM_GENERIC 5    /* K % 32 != 0, or any other patch size: 64 x 128, per-element addresses */
#define CLIPFS_GEMM_PLANES64 6   /* B_planes (a_mode 0, K % 32 == 0, ldb == K): 64 x 128 */
#define CLIPFS_GEMM_PLANES128 7  /*   128 x 128 */
struct clipfs_gemm_plan {
  int kernel;               /* CLIPFS_GEMM_* */
  int planes;               /* PLANES*: 16-bit planes per operand, 2 (bf16 hi / lo) or 1 (f16); 0 otherwise */
  int tile_rows;            /* rows of the tile that runs; MIXED: 32, the height of the tail tiles */
  int splits;               /* split-K factor granted with the scratch as given (1: unsplit) */
  int want_splits;          /* the factor the call would get with enough scratch (1 on a route that cannot split) */
  int mix_rows64;           /* MIXED: rows dealt as 64-row tiles (0 otherwise) */
  int gm;                   /* m-blocks per super-tile of the tile order */
  int grid, block;          /* workgroups, threads per workgroup */
  int lds_bytes;            /* dynamic LDS per workgroup */
  size_t workspace_floats;  /* what want_splits needs of `workspace` ... */
  size_t counter_ints;      /* ... and of `counters` (both 0 when want_splits is 1) */
};
int clipfs_gemm_plan(const clipfs_gemm_args* args, struct clipfs_gemm_plan* plan);
/* The five shape-only queries below describe a DENSE fp32 product (a_mode 0, no planes) that is given enough scratch,
 * whatever K % 32 is: they size scratch ahead of a call and keep their answers where the call then takes another route
 * (K % 32 != 0, patch mode and planes never split; those kernels exist with 64-row tiles only).  The plan is the truth
 * for a given call.  Host-only, no launch.
 * clipfs_gemm_splits: the split-K factor (the plan's want_splits). */
int clipfs_gemm_splits(int M, int N, int K);
/* rows of the block tile (64 or 32) for an [M,N] output (the plan's tile_rows) */
int clipfs_gemm_tile_rows(int M, int N);
/* Dense unsplit fp32 products of 4096 rows or more (K % 32 == 0) for which clipfs_gemm_tile_rows answers 32 may deal
 * rows [0, clipfs_gemm_mixed_rows64) as 64-row tiles -- whole rounds of the resident workgroup slots -- and only the rows
 * behind them as 32-row tiles, in one launch; 0 = one height, that of clipfs_gemm_tile_rows.  It changes no result bit: an
 * element's k order does not depend on the tile that holds it. */
int clipfs_gemm_mixed_rows64(int M, int N, int K);
/* The f16 x f16 kernel (args->A_f16 set) is nine kernels and a row split: whole rounds of 256 x 256 tiles over the CUs on
 * a ping-pong or phased kernel, the leftover rows on 4-wave kernels, on the internal side stream when `side` is set.
 * clipfs_gemm_f16_plan writes the launches clipfs_gemm_nt would make for `args` on a device of `cus` compute units
 * (cus <= 0: the current device's count; 256 when there is none) -- it IS the function the dispatch executes.  Host-only:
 * no launch, and no pointer of `args` is dereferenced (their alignment takes part in the choice).  Returns CLIPFS_EINVAL
 * for arguments clipfs_gemm_nt would refuse, or without A_f16.  The tuning aids CLIPFS_F16_TILE / _PP_FILL / _SIDE /
 * _EPILOGUE / _PHASED are read once per process and show in the plan. */
#define CLIPFS_F16_64X128 0     /* 4-wave kernels: 64 x 128 tile, three LDS stages */
#define CLIPFS_F16_64X128_S2 1  /*   64 x 128, two stages (fits beside a ping-pong workgroup) */
#define CLIPFS_F16_128X128 2
#define CLIPFS_F16_256X128 3
#define CLIPFS_F16_PP_REG 4     /* 256 x 256 ping-pong, per-lane register epilogue */
#define CLIPFS_F16_PP_LDS 5     /* 256 x 256 ping-pong, epilogue through LDS */
#define CLIPFS_F16_PH16 6       /* 256 x 256 phased on 16x16x32 MFMAs, LDS epilogue, 4 columns per thread */
#define CLIPFS_F16_PH16_WIDE 7  /*   the same with 8 columns per thread (f16-only result) */
#define CLIPFS_F16_PH32 8       /* 256 x 256 phased on 32x32x16 MFMAs */
typedef struct clipfs_f16_launch {
  int kernel;            /* CLIPFS_F16_* */
  int m_begin, m_end;    /* rows [m_begin, m_end) of the problem */
  int side;              /* 1: on the side stream */
} clipfs_f16_launch;
typedef struct clipfs_f16_plan {
  int n;                 /* launches, 1 .. 3, in row order */
  clipfs_f16_launch launch[3];
} clipfs_f16_plan;
int clipfs_gemm_f16_plan(const clipfs_gemm_args* args, int cus, clipfs_f16_plan* out);
/* floats of `workspace` and ints of `counters` the split of clipfs_gemm_splits needs: one slab of a whole tile per K slice
 * and tile, one arrival counter per tile (the plan's workspace_floats / counter_ints); 0 for a shape that does not split.
 * The opt-in stream-K schedule that also used them (CLIPFS_GEMM_SK) was removed at this commit: it lost inside the step. */
size_t clipfs_gemm_workspace_floats(int M, int N, int K);
size_t clipfs_gemm_counter_ints(int M, int N, int K);
/* Diagnostics for bench.py's roofline leg (never enabled inside a timed region): while enabled, every
 * GEMM launch of the calling thread is bracketed by HIP events on its launch stream;
 * clipfs_gemm_timing_collect synchronises on them and returns the summed kernel time, the summed
 * algorithmic FLOPs (2*M*N*K) and the number of launches since the last collect. */
int clipfs_gemm_timing(int enable);
int clipfs_gemm_timing_collect(double* total_ms, double* total_flops, int* launches);
/* algorithmic HBM bytes (every operand, result and epilogue tensor counted once) of the launches summed by the last
 * clipfs_gemm_timing_collect of the calling thread */
double clipfs_gemm_timing_last_bytes(void);

/* ------------------------------------------------------------- LayerNorm --
 * y = (x - mean) / sqrt(var + eps) * gamma + beta over the last dim (biased var).
 * Replaces jittor nn.LayerNorm, jclip/model.py:17-21,115,121,209.
 * `x` rows are read with stride ldx (lets ln_post read the class-token rows in place).
 * mean/rstd (each [rows]) may be NULL (inference). */
int clipfs_layernorm_fwd(const float* x, int ldx, const float* gamma, const float* beta, float* y,
                         float* mean, float* rstd, int rows, int width, float eps, void* stream);
/* dx = dres + LN'(dy)   (dres may be NULL); gamma frozen: no dgamma/dbeta. */
int clipfs_layernorm_bwd(const float* dy, const float* x, int ldx, const float* gamma, const float* mean,
                         const float* rstd, const float* dres, float* dx, int lddx, int rows, int width,
                         void* stream);
/* The same backward with x, mean and rstd read at row xmap[r] for output row r (dy, dres, dx stay dense [rows, ...]):
 * the packed text backward reads the forward's full-layout tensors in place.  Arithmetic identical per row. */
int clipfs_layernorm_bwd_rows(const float* dy, const float* x, int ldx, const float* gamma, const float* mean,
                              const float* rstd, const int32_t* xmap, const float* dres, float* dx, int lddx, int rows,
                              int width, void* stream);
/* fp16 storage mode: the same kernels writing an f16 copy of the result [rows, width] for the GEMM that consumes it
 * (y16 / dx16 may be NULL; in the forward y may be NULL when only the f16 operand is needed). */
int clipfs_layernorm_fwd_f16(const float* x, int ldx, const float* gamma, const float* beta, float* y, void* y16,
                             float* mean, float* rstd, int rows, int width, float eps, void* stream);
int clipfs_layernorm_bwd_f16(const float* dy, const float* x, int ldx, const float* gamma, const float* mean,
                             const float* rstd, const float* dres, float* dx, void* dx16, int lddx, int rows, int width,
                             void* stream);
/* clipfs_layernorm_bwd_rows with the f16 copy of clipfs_layernorm_bwd_f16: x, mean and rstd read at row xmap[r], dy,
 * dres, dx and dx16 (may be NULL) dense [rows, ...].  The fp16 storage mode's packed text backward; the arithmetic per
 * row is that of both siblings, and dres may alias dx. */
int clipfs_layernorm_bwd_rows_f16(const float* dy, const float* x, int ldx, const float* gamma, const float* mean,
                                  const float* rstd, const int32_t* xmap, const float* dres, float* dx, void* dx16, int lddx,
                                  int rows, int width, void* stream);
/* LayerNorm forward with the adapter's down-projection in the same pass: y = LN(x) (and / or its f16 copy y16) and
 * t[row, s*r + j] = sum_k dropout_s(y)[row, k] * A[s*r + j, k], exactly clipfs_layernorm_fwd(_f16) followed by
 * clipfs_lora_down on y (same Philox counters, so clipfs_lora_bwd regenerates the same masks; t agrees to fp32 summation
 * order).  Replaces ln_1 + lora_A(dropout(x)) of the adapted q/k/v projections, jclip/model.py:115 with
 * lora_train_vlp.py:296-306.  Covered: nseg == 3, r in {1, 2, 4} (clipfs_layernorm_fwd_lora_ok); other shapes take the
 * two separate calls.  keep_bits (may be NULL): as for clipfs_lora_down. */
int clipfs_layernorm_fwd_lora_ok(int width, int r, int nseg);
int clipfs_layernorm_fwd_lora(const float* x, int ldx, const float* gamma, const float* beta, float* y, void* y16,
                              float* mean, float* rstd, int rows, int width, float eps, const float* A, float* t, int r,
                              int nseg, unsigned seg_mask, float p, uint64_t seed, uint32_t stream_base, uint32_t drow0,
                              void* keep_bits, void* stream);
/* The same with the dropout masks of row i drawn at row drow0 + drow_map[i] (int32, device, [rows]): the live-row text
 * forward runs packed rows and draws the masks (and records the keep bits) of their full-layout rows. */
int clipfs_layernorm_fwd_lora_map(const float* x, int ldx, const float* gamma, const float* beta, float* y, void* y16,
                                  float* mean, float* rstd, int rows, int width, float eps, const float* A, float* t, int r,
                                  int nseg, unsigned seg_mask, float p, uint64_t seed, uint32_t stream_base, uint32_t drow0,
                                  const int32_t* drow_map, void* keep_bits, void* stream);

/* ------------------------------------------------------------- attention --
 * qkv [B*L, 3*d] (q | k | v, head h at columns h*64..), out [B*L, d] heads merged.
 * out = softmax(q k^T / sqrt(64) + causal mask) v per (b, head), head_dim = 64.
 * Replaces scaled_dot_product_attention + reshapes + permute(2,0,1,3):
 * jclip/mha.py:55-83,439-458 and lora_train_vlp.py:339-367,492-501.
 * Scores/probabilities never leave the CU (reference: [N*H,L,L] round trip in HBM). */
int clipfs_attention_fwd(const float* qkv, float* out, float* lse, int batch, int seq, int heads, int causal,
                         void* stream);
/* dqkv from dout, recomputing the probabilities from qkv.
 * Default path, seq <= clipfs_attention_mfma_max_seq(): exact-fp32 MFMA kernels (scores kept transposed so that the
 * softmax statistics are per-lane scalars).  Up to 96 tokens 16-token tiles with every operand in LDS; up to 288 tokens
 * one workgroup of 32-token tiles takes a (batch, head) with the other side's transposed image whole in LDS; past that the
 * own side is cut into runs of 32-token tiles, one workgroup each, and the other side passes through LDS in chunks of at
 * most 288 tokens -- the same tile arithmetic in the same order, every output element written by one wave, so results are
 * bitwise reproducible at every length.  The forward writes lse [clipfs_attention_lse_floats = batch * heads * seq]
 * (log-sum-exp of the scaled scores per (batch, head, query)) when given the buffer -- no kernel is chosen by it; the
 * backward takes the forward's `out`, that `lse` and a `work` buffer of the same size.
 * What the MFMA kernels decline -- seq > clipfs_attention_mfma_max_seq() (up to 4096), an out / dqkv that is not 16-byte
 * aligned (same function, not the same bits), CLIPFS_ATTN_MFMA=0 at every length -- runs on streaming VALU kernels with
 * an online softmax.  A backward without out, lse or work: seq <= 96 runs a VALU kernel that recomputes the softmax,
 * seq > 96 is refused.  clipfs_attention_plan tells which of these a call gets. */
int clipfs_attention_bwd(const float* qkv, const float* dout, const float* out, const float* lse, float* dqkv,
                         float* work, int batch, int seq, int heads, int causal, void* stream);
size_t clipfs_attention_lse_floats(int batch, int seq, int heads);
/* The dispatch of the five entry points as data: clipfs_attention_plan IS the function they execute.  Host-only (no GPU
 * is opened, nothing is launched).  Returns CLIPFS_EINVAL with the refusal's message for what the entry point would
 * refuse.  The aids CLIPFS_ATTN_MFMA=0 (streaming kernels at every length) and CLIPFS_ATTN16=0 (32-token tiles below 97
 * tokens too, no packed kernels) are read once per process and show in the plan. */
#define CLIPFS_ATTN_FWD 0             /* direction: clipfs_attention_fwd */
#define CLIPFS_ATTN_BWD 1             /*   clipfs_attention_bwd */
#define CLIPFS_ATTN_FWD_PACKED 2      /*   clipfs_attention_fwd_packed */
#define CLIPFS_ATTN_BWD_PACKED 3      /*   clipfs_attention_bwd_packed (dense records) */
#define CLIPFS_ATTN_BWD_PACKED_IO 4   /*   clipfs_attention_bwd_packed_io (packed records) */
#define CLIPFS_ATTN_STATS 1           /* flag: backward has out, lse and work (forward: lse asked for; changes nothing) */
#define CLIPFS_ATTN_ALIGNED 2         /* flag: out / dqkv are 16-byte aligned */
#define CLIPFS_ATTN_MFMA16 0          /* family: 16-token-tile MFMA, `nt` tiles (seq <= 96) */
#define CLIPFS_ATTN_MFMA16_PACKED 1   /*   ... on live rows, records dense */
#define CLIPFS_ATTN_MFMA16_PINNED 2   /*   ... on live rows, records packed too */
#define CLIPFS_ATTN_MFMA32 3          /*   32-token-tile MFMA, one workgroup per head (seq <= 288) */
#define CLIPFS_ATTN_MFMA_LONG 4       /*   the same tiles in `parts` runs of `tiles`, other side in chunks of `ctok` */
#define CLIPFS_ATTN_STREAM 5          /*   streaming VALU */
#define CLIPFS_ATTN_RECOMPUTE 6       /*   softmax-recomputing VALU backward, instance `lmax` (64, 80, 96) */
struct clipfs_attention_launch {
  unsigned grid_x, grid_y, block, lds_bytes; /* lds_bytes: dynamic LDS */
};
struct clipfs_attention_plan {
  int family;               /* CLIPFS_ATTN_* family */
  int nt;                   /* MFMA16*: 16-token tiles, 1 .. 6 (0 otherwise, as the next four) */
  int parts, tiles, ctok;   /* MFMA_LONG: the cut */
  int lmax;                 /* RECOMPUTE */
  int launches;             /* 1 or 2 */
  struct clipfs_attention_launch launch[2];
};
int clipfs_attention_plan(int direction, int batch, int seq, int heads, int causal, int flags,
                          struct clipfs_attention_plan* plan);
/* Longest sequence the exact-fp32 MFMA attention takes (1024). */
int clipfs_attention_mfma_max_seq(void);
/* The long-sequence MFMA kernels with an explicit cut, for any 96 < seq <= clipfs_attention_mfma_max_seq() (the default
 * dispatch launches them past 288 tokens with chunk_tokens = run_tiles = 0): the other side passes through LDS in chunks
 * of at most chunk_tokens tokens (a multiple of 32, <= 288; 0 = 288), the own side is cut into runs of at most run_tiles
 * 32-token tiles (1 .. 4; 0 = 4), both evened out over the sequence.  Neither changes a bit of the result: for
 * seq <= 288 it is the result of clipfs_attention_fwd / _bwd.  lse may be NULL in the forward; the backward needs out, lse
 * and work (batch*heads*seq floats).  CLIPFS_EINVAL (nothing launched) for a seq, chunk_tokens or run_tiles outside
 * those ranges and for a NULL or misaligned pointer, the message naming the argument. */
int clipfs_attention_mfma_long_fwd(const float* qkv, float* out, float* lse, int batch, int seq, int heads, int causal,
                                   int chunk_tokens, int run_tiles, void* stream);
int clipfs_attention_mfma_long_bwd(const float* qkv, const float* dout, const float* out, const float* lse, float* dqkv,
                                   float* work, int batch, int seq, int heads, int causal, int chunk_tokens, int run_tiles,
                                   void* stream);
/* Packed (live-row) causal backward of the text tower, seq <= 96 on the exact-fp32 16-token-tile kernels
 * (clipfs_attention_bwd_packed_ok(seq, causal) != 0; needs causal and the MFMA kernels).  Sequence b is live on tokens
 * 0 .. Lb - 1, Lb = off[b + 1] - off[b] in [1, seq] (off: int32 [batch + 1], device, off[0] = 0): qkv, out and lse are the
 * forward's full-layout tensors (row b * seq + tok), dout and dqkv are packed [off[batch], d] / [off[batch], 3 d] (row
 * off[b] + tok).  Each live row gets exactly the values the full-layout call computes when every dead row of dout is 0;
 * tiles past Lb do no work. */
int clipfs_attention_bwd_packed_ok(int seq, int causal);
int clipfs_attention_bwd_packed(const float* qkv, const float* dout, const float* out, const float* lse, float* dqkv,
                                const int32_t* off, int batch, int seq, int heads, void* stream);
/* The live-row causal forward on the same kernels (clipfs_attention_bwd_packed_ok): qkv [off[batch], 3 d] and out
 * [off[batch], d] packed, lse (may be NULL) in its [batch * heads][seq] layout with entries past Lb left unwritten.  Each
 * live row gets bitwise the values of the full-layout clipfs_attention_fwd (a dead key gets weight 0 from a live query).
 * The backward over what it wrote: clipfs_attention_bwd_packed_io, which also reads qkv and out packed. */
int clipfs_attention_fwd_packed(const float* qkv, float* out, float* lse, const int32_t* off, int batch, int seq, int heads,
                                void* stream);
int clipfs_attention_bwd_packed_io(const float* qkv, const float* dout, const float* out, const float* lse, float* dqkv,
                                   const int32_t* off, int batch, int seq, int heads, void* stream);
/* fp16 storage mode (cfg-5), seq <= clipfs_attention_f16_max_seq(): the same function with both contractions on
 * v_mfma_f32_32x32x16_f16 (operands rounded to f16 in the staging path; softmax statistics, accumulators and
 * outputs fp32).  lse as above (may be NULL when no backward follows).
 * Up to 288 tokens one workgroup takes a (batch, head) with the other side resident in LDS; past that (ViT-L/14 at 336 px
 * has 577 tokens) the own side is cut into runs of 32-token tiles and the other side passes through LDS in chunks.
 * Every output element is written by one workgroup, so results are bitwise reproducible at every length.
 * clipfs_attention_f16_plan tells which of the two a call gets, with its cut, grids and LDS bytes.  This family has no
 * fallback: a longer seq, a NULL or a misaligned pointer is refused before anything is launched. */
int clipfs_attention_f16_max_seq(void);
/* The dispatch of the three entry points below as data: clipfs_attention_f16_plan IS the function they execute, under
 * the contract of clipfs_attention_plan (host-only, nothing written to `plan` on refusal, a NULL `plan` refused).
 * flags: CLIPFS_ATTN_STATS (backward: out, lse and work are there; the forward's plan does not depend on it) and
 * CLIPFS_ATTN_ALIGNED (every pointer the entry point checks is 16-byte aligned).  nt and lmax stay 0. */
#define CLIPFS_ATTN_F16_FWD 0         /* direction: clipfs_attention_f16_fwd */
#define CLIPFS_ATTN_F16_BWD 1         /*   clipfs_attention_f16_bwd */
#define CLIPFS_ATTN_F16_BWD_PACKED 2  /*   clipfs_attention_f16_bwd_packed */
#define CLIPFS_ATTN_F16_SHORT 7       /* family: one workgroup per (batch, head), seq <= 288 */
#define CLIPFS_ATTN_F16_LONG 8        /*   `parts` runs of `tiles` 32-token tiles, other side in chunks of `ctok` */
int clipfs_attention_f16_plan(int direction, int batch, int seq, int heads, int causal, int flags,
                              struct clipfs_attention_plan* plan);
int clipfs_attention_f16_fwd(const void* qkv, int qkv_f16, float* out, void* out16, float* lse, int batch, int seq,
                             int heads, int causal, void* stream);
/* dqkv from (qkv, dout, out, lse) of clipfs_attention_f16_fwd; work: batch*heads*seq floats (D_i = dO_i . O_i).
 * out16 / dqkv16 (may be NULL): f16 copies of out / dqkv, the A operands of the GEMMs that follow; with dqkv16 given,
 * dqkv itself may be NULL (fp16 storage mode: every consumer reads the f16 image, see clipfs_lora_bwd_f16dy).
 * qkv_f16 != 0: qkv is an f16 tensor [B*L, 3*d] (the QKV GEMM's f16 output: fp16 storage), else fp32.
 * dout_f16 != 0: dout is an f16 tensor [B*L, d] (the output-projection dgrad GEMM's f16-only result), else fp32. */
int clipfs_attention_f16_bwd(const void* qkv, int qkv_f16, const void* dout, int dout_f16, const float* out,
                             const float* lse, float* dqkv, void* dqkv16, float* work, int batch, int seq, int heads,
                             int causal, void* stream);
/* Packed (live-row) causal backward of the text tower in fp16 storage mode, on the one-workgroup-per-head kernels
 * above (clipfs_attention_f16_bwd_packed_ok(seq, causal) != 0: the CLIPFS_ATTN_F16_BWD_PACKED plan succeeds).
 * As clipfs_attention_bwd_packed: sequence b is live on tokens 0 .. Lb - 1, Lb = off[b + 1] - off[b] in [1, seq]; qkv (fp32 or f16), out and lse are the
 * dense forward's tensors (row b * seq + tok, lse [b * heads + h][seq]) and work keeps that dense layout; dout (fp32 or
 * f16) and dqkv / dqkv16 are packed (row off[b] + tok).  Either of dqkv / dqkv16 may be NULL, not both.  Each live row
 * gets exactly the values clipfs_attention_f16_bwd computes when every dead row of dout is 0, in both images; tiles past
 * Lb do no work. */
int clipfs_attention_f16_bwd_packed_ok(int seq, int causal);
int clipfs_attention_f16_bwd_packed(const void* qkv, int qkv_f16, const void* dout, int dout_f16, const float* out,
                                    const float* lse, float* dqkv, void* dqkv16, float* work, const int32_t* off, int batch,
                                    int seq, int heads, void* stream);

/* ------------------------------------------------------------------ LoRA --
 * t[m, s*r + j] = sum_k drop_s(x)[m,k] * A[s*r + j, k]       (the "down" half of
 * lora_train_vlp.py:302: x @ (B@A)^T == (x @ A^T) @ B^T; the reference materialises B@A).
 * drop_s = Philox dropout of nn.Dropout(p) (:298-299), one independent stream per
 * segment s: stream id = stream_base + s, element (drow0 + m, k) as documented in DESIGN.md
 * (drow0 = index of row 0 in the GLOBAL batch: a data-parallel shard draws the masks of the
 * one-process run); p = 0 or seed == 0 disables dropout.  seg_mask bit s = 0 leaves t[:, s*r..] = 0.
 * Two kernel families run these calls, the matrix-core kernels (ranks 1 ... 64) and the one-wave-per-row kernels;
 * clipfs_lora_plan below is the function that chooses, and says for any shape what runs or why it is refused.  A rank
 * no family takes is CLIPFS_EINVAL, the message naming the rank and the width. */
int clipfs_lora_down(const float* x, const float* A, float* t, int rows, int width, int r, int nseg,
                     unsigned seg_mask, float p, uint64_t seed, uint32_t stream_base, uint32_t drow0,
                     void* keep_bits, void* stream);
/* keep_bits (may be NULL): uint16 [rows, width/4]; with dropout active the forward records its masks there -- bit
 * 4*s + e of entry (m, c) set <=> element (m, 4*c + e) was kept for segment s -- and clipfs_lora_bwd / _f16dy given the
 * same buffer read them instead of evaluating Philox again (identical masks by construction; the adapter's dA / dx
 * products were VALU-bound on the generator).  Matrix-core kernels only: clipfs_lora_keep_bits_ok(...) != 0, the
 * plan's keep_bits_ok (4 bits per segment and float4 at every rank). */
int clipfs_lora_keep_bits_ok(int width, int segw, int r, int nseg);
/* The dispatch of the four entry points as data: clipfs_lora_plan IS the function they execute.  Host-only (no GPU is
 * opened, nothing is launched).  Returns CLIPFS_EINVAL with the entry point's own message, which names the cause, for
 * a shape the entry point would refuse.  The aids CLIPFS_LORA_MFMA=0 (one-wave-per-row kernels only) and
 * CLIPFS_LORA_KEEP_BITS=0 (no keep bits) are read once per process and show in the plan.  The matrix-core family takes
 * 1 <= r <= 64, nseg 1 or 3, width % 128 == 0 and segw % 64 == 0; what it declines goes to the row family: a
 * down-projection of nseg * r <= 64 outputs at width <= 2048, a backward of rank 1, 2, 4, 8 or 16. */
#define CLIPFS_LORA_OP_DOWN 0          /* operation: clipfs_lora_down (segw is not looked at) */
#define CLIPFS_LORA_OP_BWD 1           /*   clipfs_lora_bwd, clipfs_lora_bwd_xact */
#define CLIPFS_LORA_OP_BWD_F16DY 2     /*   clipfs_lora_bwd_f16dy */
#define CLIPFS_LORA_FLAG_X_ACT 1       /* flag: x holds the pre-activation (clipfs_lora_bwd_xact with x_act = 1) */
#define CLIPFS_LORA_FLAG_KEEP_BITS 2   /*   keep_bits given */
#define CLIPFS_LORA_FLAG_FROZEN 4      /*   dA == dB == NULL */
#define CLIPFS_LORA_FLAG_DX 8          /*   dx given */
#define CLIPFS_LORA_FAMILY_MFMA 0      /* family: matrix-core kernels, `groups` rank groups of 16 */
#define CLIPFS_LORA_FAMILY_ROW 1       /*   one-wave-per-row kernels */
struct clipfs_lora_launch {
  unsigned grid_x, grid_y, block;
};
struct clipfs_lora_plan {
  int family;                 /* CLIPFS_LORA_FAMILY_* */
  int groups, rq;             /* MFMA: the instance -- rank groups G = ceil(r / 16); K-steps RQ of the dA / dx launch,
                                 ceil(r / 4) up to r = 16 and 4 G above (0 in the row family and for the down-projection) */
  int sr_b, slices_b;         /* backward: rows per slice and slices of the dB reduction (no slices when frozen) */
  int sr_a, slices_a;         /*   ... of the dA reduction */
  size_t work_floats;         /* floats the call writes into `work`: the dB partials [slices_b][nseg * segw][r], then */
  size_t part_a_offset;       /*   from this offset the dA partials [slices_a][nseg * r][width] */
  int keep_bits_ok, f16dy_ok; /* whether the shape may record / read keep bits, and take dy as its f16 image */
  int launches;               /* MFMA backward: dB partials || dt, dA partials || dx, both slice sums.  Row backward: dt,
                                 dB partials, sum, dA partials, sum, dx.  Frozen or without dx: those launches are absent */
  struct clipfs_lora_launch launch[6];
};
int clipfs_lora_plan(int op, int rows, int width, int segw, int r, int nseg, int flags, struct clipfs_lora_plan* plan);
/* Backward of the adapter pair for one linear with nseg stacked segments:
 *   dt[m, s*r+j]  = scale * sum_n dy[m, s*segw + n] * B[s*segw + n, j]
 *   dB[s*segw+n,j] += scale * sum_m dy[m, s*segw+n] * t[m, s*r+j]
 *   dA[s*r+j, k]  += sum_m dt[m, s*r+j] * drop_s(x)[m,k]
 *   dx[m,k]       += sum_{s,j} dt[m, s*r+j] * A[s*r+j,k] * dropscale_s(m,k)   (if dx != NULL)
 * work: caller scratch, >= clipfs_lora_bwd_work_floats(...) floats: a bound over the families that may take the call
 * (the plan's work_floats is what the call writes).  dy, x, A, work and dx must be 16-byte aligned in all three backward
 * entry points: a misaligned one is CLIPFS_EINVAL ("misaligned pointer"), never another kernel family.
 * Frozen adapter: dA == dB == NULL computes dt and the dx contribution only -- no dB / dA partial products or slice
 * reductions are launched, and dt / dx are bitwise those of the call with slots.  With dx NULL as well only dt is
 * computed.  Exactly one of dA / dB NULL is CLIPFS_EINVAL.  The same holds for clipfs_lora_bwd_f16dy. */
size_t clipfs_lora_bwd_work_floats(int rows, int width, int r, int nseg);
int clipfs_lora_bwd(const float* dy, const float* x, const float* t, const float* A, const float* B,
                    float* dt, float* dA, float* dB, float* dx, int rows, int width, int segw, int r,
                    int nseg, unsigned seg_mask, float scale, float p, uint64_t seed, uint32_t stream_base,
                    uint32_t drow0, const void* keep_bits, float* work, void* stream);
/* Rectangular adapters (nseg == 1 only): clipfs_lora_bwd also takes segw != width -- width the adapter's input width,
 * segw its output width (dy [rows, segw], B [segw, r], A [r, width]; both multiples of 4) -- the MLP linears' d -> 4d and
 * 4d -> d.  Their work buffer is sized by clipfs_lora_bwd_work_floats2, which equals
 * clipfs_lora_bwd_work_floats for segw == width.  clipfs_lora_down takes widths up to 4096 (c_proj's input).
 * clipfs_lora_bwd_xact is the one-segment call (seg_mask 1, no keep bits) with a switch on how x is read: x_act = 1 says x
 * holds a pre-activation u and the adapter's input was QuickGELU(u), which the dA product applies as it loads x -- the
 * c_proj adapter, whose forward saves u alone; dx then receives the gradient wrt QuickGELU(u).  x_act = 0 reads x as is.
 * clipfs_gelu_bwd_inplace: dg[i] *= dQuickGELU(u[i]) for i < n (16-byte accesses, any n; pointers 16-byte aligned) -- the
 * step that follows when the c_proj dgrad GEMM ran without act = 2 so that the adapter's term could be added first. */
size_t clipfs_lora_bwd_work_floats2(int rows, int width, int segw, int r, int nseg);
int clipfs_lora_bwd_xact(const float* dy, const float* x, const float* t, const float* A, const float* B, float* dt,
                         float* dA, float* dB, float* dx, int rows, int width, int segw, int r, float scale, float p,
                         uint64_t seed, uint32_t stream_base, uint32_t drow0, int x_act, float* work, void* stream);
int clipfs_gelu_bwd_inplace(float* dg, const float* u, size_t n, void* stream);
/* The same with dy given as its f16 image [rows, nseg*segw] (fp16 storage mode: the tensor the dgrad GEMM consumes), so
 * that the two passes over dy move half the bytes and the fp32 dy need not exist.  Matrix-core kernels only:
 * clipfs_lora_bwd_f16dy_ok(width, segw, r, nseg) != 0, the plan's f16dy_ok, says a shape is covered. */
int clipfs_lora_bwd_f16dy_ok(int width, int segw, int r, int nseg);
int clipfs_lora_bwd_f16dy(const void* dy16, const float* x, const float* t, const float* A, const float* B,
                          float* dt, float* dA, float* dB, float* dx, int rows, int width, int segw, int r,
                          int nseg, unsigned seg_mask, float scale, float p, uint64_t seed, uint32_t stream_base,
                          uint32_t drow0, const void* keep_bits, float* work, void* stream);

/* --------------------------------------------------------- token assembly --
 * vit: x[b,0,:] = class_embedding + pos[0]; x[b, 1+P+i, :] = vpt[i]  (jclip/model.py:109-114,
 * jclip/model1.py:192-194).  Patch rows are written by the patch GEMM epilogue. */
int clipfs_vit_fill_special(float* x, const float* class_emb, const float* pos, const float* vpt, int batch,
                            int tokens, int n_patch, int n_vpt, int width, void* stream);
/* text: x[c,l,:] = (ctx row if 1 <= l <= n_ctx and ctx != NULL else table[ids[c,l]]) + pos[l]
 * (jclip/model.py:203-205; slow_pace.py:185-199,838). */
int clipfs_text_embed(const int64_t* ids, const float* table, const float* pos, const float* ctx, int n_ctx,
                      float* x, int n, int seq, int width, void* stream);
/* dtok[i,:] += sum_c dx[c, first+i, :]: gradient of tokens shared by every sequence -- the text prompt
 * ctx (first = 1, slow_pace.py:198-199) or the VPT tokens (first = 1 + patches, model1.py:192-194). */
int clipfs_token_rows_grad(const float* dx, float* dtok, int n, int seq, int width, int n_tok, int first,
                           void* stream);
/* C[m,n] = alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn]: strided VALU product for the two tiny
 * logits-backward products whose reduction runs over the classes (403: not 16-byte friendly). */
int clipfs_matmul_small(const float* A, const float* B, float* C, int M, int N, int K, long sam, long sak,
                        long sbk, long sbn, float alpha, void* stream);
/* out[c,:] = x[c*seq + argmax_l ids[c,l], :]   (EOT row, jclip/model.py:213-214) ; idx_out optional */
int clipfs_gather_eot(const float* x, const int64_t* ids, float* out, int32_t* idx_out, int n, int seq,
                      int width, void* stream);
/* scatter-add of the above: dx[c*seq + idx[c], :] = dy[c,:], all other rows zero */
int clipfs_scatter_rows(const float* dy, const int32_t* idx, float* dx, int n, int seq, int width, void* stream);
/* one row per sequence, the building blocks of the sparse last-block backward (clipfs_tower_bwd_sparse):
 *   gather:  out[c, :] = src[(c*seq + idx[c]) * ld + 0..width)          add:  dx[c*seq + idx[c], :] += src[c, :] */
int clipfs_gather_seq_rows(const float* src, size_t ld, const int32_t* idx, float* out, int n, int seq, int width,
                           void* stream);
int clipfs_add_seq_rows(const float* src, const int32_t* idx, float* dx, int n, int seq, int width, void* stream);
/*   put:     dst[(c*seq + idx[c]) * ld + 0..width) = src[c, :]  (other rows untouched; clipfs_tower_fwd_rows)
 *   eot_index: idx[c] = argmax_l ids[c, l], first maximum (the EOT position, jclip/model.py:213-214) */
int clipfs_put_seq_rows(const float* src, const int32_t* idx, float* dst, size_t ld, int n, int seq, int width,
                        void* stream);
int clipfs_eot_index(const int64_t* ids, int32_t* idx, int n, int seq, void* stream);
/* rows through a map (the packed text backward): gather  out[i, :] = src[map[i] * ld + 0..width)   (i < n)
 *                                                 put     dst[map[i] * ld + 0..width) = src[i, :] (other rows untouched) */
int clipfs_gather_rows_map(const float* src, size_t ld, const int32_t* map, float* out, int n, int width, void* stream);
int clipfs_put_rows_map(const float* src, const int32_t* map, float* dst, size_t ld, int n, int width, void* stream);
/* gather / put for a tensor kept as f16 (the saved pre-GELU activation of the fp16 storage mode); ld in halves, the
 * compact side [n, width] is fp32 */
int clipfs_gather_seq_rows_f16(const void* src_f16, size_t ld, const int32_t* idx, float* out, int n, int seq, int width,
                               void* stream);
int clipfs_put_seq_rows_f16(const float* src, const int32_t* idx, void* dst_f16, size_t ld, int n, int seq, int width,
                            void* stream);

/* --------------------------------------------------------- BPE tokenizer --
 * Native merge loop of the CLIP byte-pair encoder (jclip/simple_tokenizer.py:88-129; host code, no GPU work).
 * create: `merges` = the merges text after its header line, one "left right" per line; returns an opaque handle or
 * NULL.  encode: word w = UTF-8 bytes [offsets[w], offsets[w+1]) of `words` (already cleaned, lower-cased and split by
 * the caller); writes each word's vocabulary ids consecutively into ids (capacity cap) and their number into
 * counts[w]; returns the total or -1. */
void* clipfs_bpe_create(const char* merges, size_t n_bytes, int n_merges);
void clipfs_bpe_destroy(void* handle);
long clipfs_bpe_encode(const void* handle, const uint8_t* words, const int32_t* offsets, int n_words, int32_t* ids,
                       int32_t* counts, long cap);

/* ------------------------------------------------- MoCo ResNet-50 branch --
 * Data movement of the frozen ResNet-50 feature extractor (slow_pace.py:1237-1271,1677-1680; forward only, NHWC
 * activations; convolutions run as clipfs_gemm_nt with BatchNorm folded into weights / bias and ReLU = act 3):
 *   nchw_to_nhwc : y[n,h,w,c] = x[n,c,h,w]
 *   im2col_nhwc  : col[(n,ho,wo), (ky,kx,c)] = x[n, ho*stride-pad+ky, wo*stride-pad+kx, c] (0 outside), row length Kp
 *                  (>= kh*kw*C, multiple of 4, tail zero) -- the A operand of the convolution's GEMM
 *   maxpool3x3s2 : torchvision's MaxPool2d(3, 2, 1) on NHWC;   global_avgpool : mean over HW -> [N, C] */
int clipfs_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, void* stream);
int clipfs_im2col_nhwc(const float* x, float* col, int N, int H, int W, int C, int kh, int kw, int stride, int pad,
                       int Kp, void* stream);
int clipfs_maxpool3x3s2_nhwc(const float* x, float* y, int N, int H, int W, int C, void* stream);
int clipfs_global_avgpool_nhwc(const float* x, float* y, int N, int HW, int C, void* stream);

/* ------------------------------------------------ CLIP ModifiedResNet tower --
 * What CLIP's ModifiedResNet (RN50 family) needs beside the kernels above (forward only, fp32, NHWC; every pointer
 * 16-byte aligned, C a multiple of 4; bad arguments return CLIPFS_EINVAL before anything is launched):
 *   avgpool_nhwc    : y [N, H/k, W/k, C] = k x k mean with stride k, no padding, sizes floored (rows / columns past the
 *                     last full window are never read); sum order row-major inside the window.  1 <= k <= min(H, W).
 *   attnpool_tokens : x [N, HW, C], pos [HW+1, C] -> tok [N, HW+1, C]:  tok[n,0] = mean_i x[n,i] + pos[0],
 *                     tok[n,1+i] = x[n,i] + pos[1+i]; one pass over x, the mean summed in ascending i.
 *   attnpool_attend : q [N, heads*64], kv [N*L, 2*heads*64] (k | v) -> out [N, heads*64] = softmax_j(q.k_j / 8) . v_j per
 *                     (image, head): the pool's single query row.  Max-subtracted softmax, fp32.  2 <= L <= 1024,
 *                     1 <= heads <= 128. */
int clipfs_avgpool_nhwc(const float* x, float* y, int N, int H, int W, int C, int k, void* stream);
int clipfs_attnpool_tokens(const float* x, const float* pos, float* tok, int N, int HW, int C, void* stream);
int clipfs_attnpool_attend(const float* q, const float* kv, float* out, int N, int L, int heads, void* stream);

/* ---------------------------------------------------------- head / loss --
 * y = x / ||x||_2 per row; inv_norm[row] saved (may be NULL).  jclip/model.py:222-224. */
int clipfs_l2norm_fwd(const float* x, float* y, float* inv_norm, int rows, int width, void* stream);
/* dx = inv_norm * (dy - y * <dy,y>) */
int clipfs_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int rows, int width,
                      void* stream);
/* per class: normalise each template embedding, mean, normalise (lora_train_vlp.py:978-990 /
 * clip_classifier :647-666).  emb [C*t, d] (class major), out [C, d]. */
int clipfs_class_mean_fwd(const float* emb, float* out, int classes, int templates, int width, void* stream);
int clipfs_class_mean_bwd(const float* emb, const float* dout, float* demb, int classes, int templates, int width,
                          void* stream);
/* mean softmax cross entropy + dlogits (= (softmax - onehot) / rows * grad_scale);
 * loss_rows [2*rows] scratch: per-sample losses, then per-row hit flags; loss_sum [1] = sum of the
 * per-sample losses (fixed summation order).  lora_train_vlp.py:997.
 * correct [1] (may be NULL) counts argmax == target (cls_acc :638-644). */
int clipfs_cross_entropy(const float* logits, const int64_t* target, float* dlogits, float* loss_rows,
                         float* loss_sum, int32_t* correct, int rows, int classes, float grad_scale,
                         void* stream);
/* top-k labels per row, ties broken towards the smaller class index (cls_acc :639, test.py:1738) */
int clipfs_topk(const float* logits, int32_t* labels, int rows, int classes, int k, void* stream);
/* Channel_LP (slow_pace.py:1195-1206): y = (scale1*x + bias1) W^T + b via clipfs_gemm_nt after this
 * affine; logit_normalize (:1276-1280): (z - rowmean)/std_all, std unbiased clamped at 1e-6.
 * work: >= 2 floats. */
int clipfs_channel_affine(const float* x, const float* scale1, const float* bias1, float* y, int rows,
                          int width, void* stream);
int clipfs_logit_normalize(const float* z, float* out, float* work, int rows, int classes, void* stream);
/* backward of logit_normalize (head training, slow_pace.py:1671-1675): dz from dzn, statistics recomputed from z */
int clipfs_logit_normalize_bwd(const float* z, const float* dzn, float* dz, int rows, int classes, void* stream);
/* out[c] = sum_r x[r,c] * (y ? y[r,c] : 1): bias / per-channel scale gradients of the head (fixed row order) */
int clipfs_colsum(const float* x, const float* y, float* out, int rows, int cols, void* stream);
/* Bias gradients: out_s[j] += sum_r x[r, s * seg_width + j] for the segments s = 0, 1, 2 of the `cols` columns
 * (cols <= 3 seg_width; seg_width <= 0 means one segment of `cols`).  x has leading dimension ldx >= cols, so a slice is
 * summed in place.  A NULL out_s is skipped (a frozen q / k / v segment of the packed in-projection bias); with every
 * segment NULL nothing is launched.  The result is ACCUMULATED into the slots, like the LoRA gradient slots.
 * Bitwise deterministic: a partial slab per row chunk, then a fixed-order pass (no float atomics).  work: >=
 * clipfs_bias_grad_work_floats(rows, cols) floats, 16-byte aligned (may be NULL when that is 0).  float4 loads when
 * cols, ldx and the base allow; the scalar form adds in the same order. */
size_t clipfs_bias_grad_work_floats(int rows, int cols);
int clipfs_bias_grad(const float* x, size_t ldx, int rows, int cols, int seg_width, float* out0, float* out1,
                     float* out2, float* work, void* stream);
/* Stage-2 self-consistency losses (slow_pace.py:1653-1658).
 * l1_loss: loss[0] = mean |a - b| (jittor nn.l1_loss); da (may be NULL) = sign(a - b) * grad_scale / n.
 * kl_logits: kl_div(log_softmax(logits), log_softmax(target_logits)) of slow_pace.py:1170-1177 per row:
 *   loss_rows[r] = sum_j q_j (log q_j - log p_j); dlogits (may be NULL) = (p - q) * grad_scale; the caller sums the rows
 *   and divides by numel (:1658). */
int clipfs_l1_loss(const float* a, const float* b, size_t n, float* loss, float* da, float grad_scale, void* stream);
int clipfs_kl_logits(const float* logits, const float* target_logits, float* loss_rows, float* dlogits, int rows,
                     int classes, float grad_scale, void* stream);
/* The stage-2 objective without its head branch (slow_pace.py:1640,1650-1658,1684-1686) in one launch plus a one-wave
 * fixed-order reduction: sim_ce = CE(cos, target) (:1686), scl_logits = kl_div(log_softmax(cos), log_softmax(zs_logits))
 * / numel (:1656-1658), scl_image = l1_loss(img, zs_img) (:1655), scl_text = l1_loss(txt, zs_txt) (:1654), and their
 * gradients, for ONE data-parallel rank: B of the B_g = 1 / inv_global_batch images and C_loc of the C classes.
 *   cos, zs_logits [B, C]   the rank's logit block and 100 * zs_img[index] * zs_txt^T; target [B] int64 in [0, C)
 *   img, zs_img    [B, d]   unit image features and their zero-shot counterparts
 *   txt, zs_txt [C_loc, d]  the unit text rows this call accounts for (C_loc = 0: none, both may be NULL)
 *   dcos [B, C]   = S * ((softmax(cos) - onehot) / B_g + (softmax(cos) - softmax(zs_logits)) / (B_g * C))
 *   dimg [B, d]   = S * sign(img - zs_img) / (B_g * d);  dtxt [C_loc, d] = S * sign(txt - zs_txt) / (C * d)
 *                   (sign(0) = 0 as clipfs_l1_loss; each of the three may be NULL = not wanted)
 *   terms [4]     = this call's SHARE of {sim_ce, scl_logits, scl_image, scl_text}: row sums over B_g, B_g * C,
 *                   B_g * d and C * d, so the shares of all ranks add up to the terms of the whole batch
 *   correct [1]   (int32, may be NULL) rows whose arg-max of cos is the target (ties to the smaller index)
 *   work          4 * B + C_loc 32-bit words: the per-row partials, added in row order (no atomics: bitwise run to run)
 * S is word CLIPFS_SCALER_SCALE of scaler_state (a loss-scaling record, see "loss scaling"), or 1 when it is NULL; it is
 * the last factor of every gradient entry, terms and correct never carry it.  A wave per row; float4 accesses where the
 * row width (C, d) is a multiple of 4 and the bases are 16-byte aligned, any C, d, B otherwise.  CLIPFS_EINVAL (nothing
 * launched) for a NULL required pointer, a misaligned pointer, a non-positive B, C, d or inv_global_batch, or C_loc
 * outside [0, C]. */
int clipfs_stage2_objective(const float* cos, const float* zs_logits, const int64_t* target, const float* img,
                            const float* zs_img, const float* txt, const float* zs_txt, float* dcos, float* dimg,
                            float* dtxt, float* work, float* terms, int32_t* correct, int B, int C, int d, int C_loc,
                            float inv_global_batch, const float* scaler_state, void* stream);

/* ------------------------------------------------------------- optimiser --
 * jittor.optim.AdamW.step (lora_train_vlp.py:946,1002): p *= 1 - lr*wd; m,v update;
 * p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps).  One launch over the flat LoRA+prompt buffer. */
int clipfs_adamw(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1,
                 float beta2, float eps, float weight_decay, float grad_scale, void* stream);

/* ---------------------------------------------------------- loss scaling --
 * For the fp16 storage mode, whose backward keeps every activation gradient as an f16 image (anything below 3e-8
 * becomes zero there): the logits gradient is multiplied by a scale S, the whole backward (linear in it) carries S, and
 * the optimiser divides it out again.  All of it is driven by a device-resident SCALER RECORD owned by the caller:
 * CLIPFS_SCALER_WORDS 32-bit words (64 bytes, 16-byte aligned), fp32 or int32 as listed, which no entry point reads
 * back to the host.  The caller initialises SCALE (> 0, a power of two keeps the scaling exact), INV_SCALE = 1 / SCALE
 * and zeroes the rest.
 *
 * One optimiser step is three launches on the caller's stream, in this order (after any gradient all-reduce, so that
 * every data-parallel rank sees the same buffer and takes the same decision):
 *   clipfs_grads_nonfinite  one pass over the flat gradient buffer [n] (any 4-byte aligned base: 16-byte loads between
 *                           the first and the last 16-byte boundary, scalar loads for the up to 3 floats on either
 *                           side); sets FOUND when an entry is NaN or +-inf.  Finite values of any magnitude
 *                           (FLT_MAX, subnormals) do not.
 *   clipfs_scaler_decide    one thread.  FOUND clear: STEP += 1; INV_SQRT_BC2 = 1 / sqrt(1 - beta2^STEP) and
 *                           STEP_SIZE = lr / (1 - beta1^STEP), evaluated in double like clipfs_adamw does on the host;
 *                           SKIP = 0; TRACKER += 1, and when growth_interval > 0 and TRACKER reaches it, SCALE *=
 *                           growth_factor (unless that overflows) and TRACKER = 0.  FOUND set: SKIPPED += 1; SKIP = 1;
 *                           SCALE *= backoff_factor; TRACKER = 0; STEP is left alone.  Either way INV_SCALE = 1 / the
 *                           scale this step's gradients carry, and FOUND = 0 for the next step.
 *                           growth_interval = 0 with backoff_factor = 1 is a static scale (it still skips).
 *                           growth_factor >= 1, 0 < backoff_factor <= 1, growth_interval >= 0.
 *   clipfs_adamw_scaled     clipfs_adamw's arithmetic with grad_scale = INV_SCALE and the two bias-correction floats
 *                           of the record; with SKIP set it writes nothing (p, m, v bitwise unchanged, no weight decay).
 * clipfs_cross_entropy_scaled is clipfs_cross_entropy with the gradient scale grad_scale * SCALE; loss_sum and correct
 * are unscaled.  Each of the four is CLIPFS_EINVAL (nothing launched) for a NULL or misaligned record or buffer or n = 0. */
#define CLIPFS_SCALER_SCALE 0        /* fp32: the scale the next cross entropy applies */
#define CLIPFS_SCALER_INV_SCALE 1    /* fp32: 1 / the scale of the step last decided */
#define CLIPFS_SCALER_FOUND 2        /* int32: a non-finite gradient entry was seen since the last decision */
#define CLIPFS_SCALER_TRACKER 3      /* int32: consecutive clean steps since the scale last changed */
#define CLIPFS_SCALER_STEP 4         /* int32: optimiser steps applied (skipped steps not counted) */
#define CLIPFS_SCALER_SKIPPED 5      /* int32: steps skipped */
#define CLIPFS_SCALER_INV_SQRT_BC2 6 /* fp32 */
#define CLIPFS_SCALER_STEP_SIZE 7    /* fp32 */
#define CLIPFS_SCALER_SKIP 8         /* int32: the step last decided is skipped */
#define CLIPFS_SCALER_WORDS 16       /* words 9 .. 15 are reserved (zero) */
int clipfs_cross_entropy_scaled(const float* logits, const int64_t* target, float* dlogits, float* loss_rows,
                                float* loss_sum, int32_t* correct, int rows, int classes, float grad_scale,
                                const float* scaler_state, void* stream);
int clipfs_grads_nonfinite(const float* g, size_t n, float* scaler_state, void* stream);
int clipfs_scaler_decide(float* scaler_state, float lr, float beta1, float beta2, float growth_factor,
                         float backoff_factor, int growth_interval, void* stream);
int clipfs_adamw_scaled(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, const float* scaler_state, void* stream);

/* ------------------------------------------------- optimiser step options --
 * Gradient clipping by global 2-norm and an exponential moving average of the parameters, in the optimiser step.
 * Clipping is driven by a device-resident CLIP RECORD owned by the caller: CLIPFS_CLIP_WORDS fp32 words (32 bytes,
 * 16-byte aligned), zeroed by the caller, which no entry point reads back to the host.  It is separate from the scaler
 * record, whose reserved words stay zero.
 *
 * With clipping one optimiser step is, on the caller's stream and after any gradient all-reduce (every data-parallel
 * rank then forms the same norm from the same bytes in the same order):
 *   [clipfs_grads_nonfinite, clipfs_scaler_decide]   with loss scaling only
 *   clipfs_grad_sumsq    pass 1 of the sum of squares of the flat gradient buffer [n] (any 4-byte aligned base: 16-byte
 *                        loads between the first and the last 16-byte boundary of each workgroup's run, scalar loads
 *                        for the up to 3 floats on either side).  Squares and sums are double: exact squares, and a
 *                        scaled gradient of 1e19 does not overflow.  Fixed-order reduction through LDS, no float
 *                        atomics; one double per workgroup goes to work [clipfs_grad_sumsq_work_doubles(n)] (8-byte
 *                        aligned).  Grid and runs depend on n alone (and the order inside a run on the base's offset
 *                        from a 16-byte boundary): the same buffer gives the same bits on every call.
 *   clipfs_clip_decide   one workgroup adds the partials of the same n in index order and writes the record:
 *                        NORM = sqrt(sum) * INV_SCALE of scaler_state (after clipfs_scaler_decide that is the scale
 *                        these gradients carry), or sqrt(sum) when it is NULL; COEF = min(1, max_norm / (NORM + 1e-6)),
 *                        the rule of torch.nn.utils.clip_grad_norm_; MULT = INV_SCALE * COEF (fp32 product), or COEF.
 *                        A NaN or infinite NORM gives COEF = 0 (torch with error_if_nonfinite=False: the non-finite
 *                        entries themselves still poison the update -- loss scaling is what skips such a step; with
 *                        its SKIP set the record still gets NORM and MULT is never used).
 *   clipfs_adamw_ext     clipfs_adamw's arithmetic on p, g, m, v [n] with three optional pointers:
 *                        scaler_state  the bias corrections, the skip decision and grad_scale = INV_SCALE come from the
 *                                      record, as in clipfs_adamw_scaled (step is then ignored);
 *                        clip_state    grad_scale = MULT of the record (it already carries INV_SCALE);
 *                        ema_shadow    [n]: shadow = fmaf(ema_decay, shadow, (1 - ema_decay) * p_new) from the parameter
 *                                      just computed, 1 - ema_decay formed once in fp32 (lora_train_vlp.py:887).
 *                        With SKIP set it writes nothing: p, m, v and the shadow stay bitwise untouched.  All three
 *                        NULL is bitwise clipfs_adamw (step, grad_scale as given); scaler_state alone is bitwise
 *                        clipfs_adamw_scaled.
 * clipfs_grad_sumsq_work_doubles is host-only, monotone in n and 0 for n = 0.  The other three are CLIPFS_EINVAL
 * (nothing launched) for a NULL or misaligned record or buffer (an optional one: misaligned), n = 0, a max_norm that
 * is not positive and finite, an ema_decay outside (0, 1) or a shadow that aliases p, m or v (shadow given), and
 * step < 1 without a scaler record. */
#define CLIPFS_CLIP_NORM 0  /* fp32: the unscaled total 2-norm of the gradients last decided */
#define CLIPFS_CLIP_COEF 1  /* fp32: min(1, max_norm / (NORM + 1e-6)); 0 for a non-finite NORM */
#define CLIPFS_CLIP_MULT 2  /* fp32: the gradient multiplier clipfs_adamw_ext applies */
#define CLIPFS_CLIP_WORDS 8 /* words 3 .. 7 are reserved (zero) */
size_t clipfs_grad_sumsq_work_doubles(size_t n);
int clipfs_grad_sumsq(const float* g, size_t n, double* work, void* stream);
int clipfs_clip_decide(const double* work, size_t n, float max_norm, const float* scaler_state, float* clip_state,
                       void* stream);
int clipfs_adamw_ext(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float grad_scale, const float* scaler_state, const float* clip_state,
                     float* ema_shadow, float ema_decay, void* stream);

/* clipfs_adamw_ext with a TAIL: the last tail_n elements of the flat buffer (i >= n - tail_n) take tail_weight_decay
 * in place of weight_decay and are clamped to [tail_min, tail_max] after the update (-inf / +inf: no bound on that
 * side); the EMA shadow sees the clamped value.  This is what a trained log-temperature needs: free of weight decay,
 * held at or below ln 100.  Same launch, same kernel; a step the scaler skips leaves the tail untouched too.
 * tail_n = 0 is bitwise clipfs_adamw_ext.  CLIPFS_EINVAL for what clipfs_adamw_ext refuses, and for tail_n > n,
 * tail_min > tail_max or a NaN bound. */
int clipfs_adamw_tail(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float grad_scale, const float* scaler_state, const float* clip_state,
                      float* ema_shadow, float ema_decay, size_t tail_n, float tail_weight_decay, float tail_min,
                      float tail_max, void* stream);

/* -------------------------------------------------------------------- MTA --
 * solve_mta (lora_train_vlp.py:742-811; slow_pace.py:1363-1433), one workgroup per image.
 * feats [n_img, V, d] unit rows (row 0 = centre view), text [C, d] (unit rows; the reference
 * passes its transpose [d, C]).  mode_out [n_img, d], logits_out [n_img, C] = 100 * mode . text
 * (either may be NULL).  work: >= clipfs_mta_work_floats floats.  views >= 5 (k = int(0.3 (V-1)) >= 1).
 * The diagonal of cdist is clamped at 0 before the sqrt (deviation from :740). */
size_t clipfs_mta_work_floats(int n_img, int views, int width, int classes);
int clipfs_mta(const float* feats, const float* text, float* mode_out, float* logits_out, float* work,
               int n_img, int views, int width, int classes, void* stream);

/* ----------------------------------------------------------- TTA views --
 * One kernel writes every normalised fp32 view [n_views, 3, S, S] of one uint8 HWC source image resident in HBM:
 * crop -> PIL-exact 8-bit resize (bilinear or bicubic, Pillow Resample.c restated) -> S x S window -> optional
 * horizontal flip -> (u8 - 255 mean) / (255 std).  Replaces the CPU/PIL view generation of ood.py:946-958,1084-1089
 * and jclip/clip.py:130-144 (Resize 256 bicubic + CenterCrop; RandomResizedCrop bilinear + RandomHorizontalFlip).
 * recs: int32 [n_views, 10] = {top, left, h, w, flip, out_w, out_h, win_x, win_y, filter(0 bilinear, 1 bicubic)};
 * boxes are sampled on the host (clipfs/views.py).  Needs max(h/out_h, w/out_w) * support * 2 + 1 <= 24 taps. */
int clipfs_tta_views(const uint8_t* image, int height, int width, const int32_t* recs, int n_views, int out_size,
                     const float* mean, const float* stdv, float* out, void* stream);

/* ------------------------------------------------------- training crops --
 * One kernel writes a whole training batch [n, 3, S, S]; each view names its own source inside ONE uint8 HWC pool of
 * decoded images (back to back in HBM).  Per view: crop -> PIL-exact 8-bit resize (bilinear or bicubic, the resampling
 * of clipfs_tta_views) -> S x S window -> optional horizontal flip.  Replaces the PIL training transform of
 * lora_train_vlp.py:1196-1218 / slow_pace.py:1903-1935 (RandomResizedCrop, RandomHorizontalFlip, ImageNormalize,
 * ToTensor).
 * pool: device, pool_bytes long.  src: int64 [n_src, 3] = {byte offset into pool, height, width}; recs: int32 [n, 12] =
 * {src index, top, left, h, w, flip, out_w, out_h, win_x, win_y, filter (0 bilinear, 1 bicubic), 0} (the box / resize /
 * window / flip meaning of clipfs_tta_views' records).  src and recs are HOST tables, validated here; src_dev and
 * recs_dev are their device copies, which the kernel reads (and re-checks against the pool, writing nothing for a view
 * that fails).  out_norm: fp32 [n, 3, S, S] = (u8 - 255 mean) * ((1 / 255) / std), the formula of clipfs_tta_views;
 * out_raw: fp32 [n, 3, S, S] = u8 / 255 (ToTensor).  Either output may be NULL, not both; both are written in one pass.
 * CLIPFS_EINVAL (nothing launched) for NULL tables, a source side outside [1, 4096] or outside the pool, a src index out
 * of range, a box outside its source, a window outside its resize, or more than 80 taps on an axis
 * (ceil(support * max(in / out, 1)) * 2 + 1). */
int clipfs_crop_batch(const uint8_t* pool, size_t pool_bytes, const int64_t* src, const int64_t* src_dev, int n_src,
                      const int32_t* recs, const int32_t* recs_dev, int n, int out_size, const float* mean,
                      const float* stdv, float* out_norm, float* out_raw, void* stream);

/* ------------------------------------------------------ merged weights --
 * Folds LoRA adapters into COPIES of the frozen weights: out = W + scale * B A, the weight the reference runs a plain
 * linear on once a layer is in eval mode (LoRALayer.merge_BA / add_lora_data, lora_train_vlp.py:218-234).  W itself is
 * read only.  ONE launch folds a whole table of projections (a tower's adapted matrices are a few MB each: a launch per
 * matrix would spend more on kernel boundaries than on bytes).
 *
 * One job = one projection:
 *   w [n, k] fp32, the master weight (read only; out must not be w);
 *   a [nseg * r, k], b [n, r]: the tower's stacked adapter layouts (qkv: nseg 3, A [3r, k], B [3d, r]; o / c_fc / c_proj:
 *     nseg 1);
 *   seg_mask: bit g set = rows g * n / nseg ... (g + 1) * n / nseg - 1 have an adapter; a clear bit = those rows of out
 *     are a bitwise copy of w;
 *   out [n, k] fp32;  planes: NULL, or the 16-bit image of out in `plane_format` (2: f16 [n, k], bit for bit what
 *     clipfs_convert_f16 makes of out; 1: bf16 hi [n, k] then lo [n, k], bit for bit clipfs_split_bf16 of out);
 *   tile0: the index of the job's first tile in the launch = the tile counts of the jobs before it, where a job has
 *     nseg * ceil(n / nseg / CLIPFS_LORA_MERGE_TILE_ROWS) * ceil(k / CLIPFS_LORA_MERGE_TILE_COLS) tiles (a tile never
 *     crosses a segment).
 * r (1 ... 64), scale and plane_format (0: no planes anywhere) are per call: one tower shares them.
 *
 * Arithmetic, fixed: for row n of segment g and column k,  acc = sum_j B[n, j] * A[g r + j, k]  in fp32, ascending j,
 * each step one fused multiply-add;  out = fma(scale, acc, W[n, k]).  No atomics, no split over j: results are
 * deterministic and  |out - (W + s B A)| <= (r + 3) 2^-24 (|W| + |s| sum_j |B A|)  elementwise.
 *
 * h_jobs is the HOST table, validated here before anything is enqueued; jobs_dev is its device copy (the same bytes,
 * uploaded by the caller), which the kernel reads.  struct_size = sizeof(clipfs_lora_merge_job) of the caller.
 * CLIPFS_EINVAL (nothing launched), the message naming the job index and the field: a struct_size this library does not
 * know, njobs <= 0, a NULL or not 16-byte aligned pointer, k % 8 != 0, nseg other than 1 or 3, n % nseg != 0, seg_mask
 * zero or outside nseg bits, out == w, planes given with plane_format 0, a wrong tile0, r outside [1, 64]. */
#define CLIPFS_LORA_MERGE_TILE_ROWS 32
#define CLIPFS_LORA_MERGE_TILE_COLS 256
typedef struct clipfs_lora_merge_job {
  const float* w;
  const float* a;
  const float* b;
  float* out;
  void* planes;
  int n, k;
  int nseg;
  unsigned seg_mask;
  int tile0;
  int reserved; /* zero */
} clipfs_lora_merge_job;
int clipfs_lora_merge(const clipfs_lora_merge_job* h_jobs, const clipfs_lora_merge_job* jobs_dev, int njobs,
                      size_t struct_size, int r, float scale, int plane_format, void* stream);

/* --------------------------------------------------------- tower drivers --
 * C++ sequencing of the kernels above for one transformer tower, so that one call
 * from Python enqueues a whole forward or backward (no per-kernel interpreter cost).
 * Replaces Transformer / ResidualAttentionBlock / VisionTransformer.execute and
 * CLIP.encode_text (jclip/model.py:42-126,202-215), PlainMultiheadAttentionLoRA
 * (lora_train_vlp.py:431-506) and their Jittor autograd. */
typedef struct clipfs_block {
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const float *w_qkv, *b_qkv, *w_qkv_t; /* [3d,d], [3d], transposed copy [d,3d] for dgrad */
  const float *w_o, *b_o, *w_o_t;       /* [d,d] */
  const float *w_fc, *b_fc, *w_fc_t;    /* [4d,d], [4d], [d,4d] */
  const float *w_pr, *b_pr, *w_pr_t;    /* [d,4d], [d], [4d,d] */
  /* LoRA on q,k,v (stacked: A [3r,d], B [3d,r]) and on the out projection (A [r,d], B [d,r]) */
  const float *lora_a_qkv, *lora_b_qkv, *lora_a_o, *lora_b_o;
  float *g_lora_a_qkv, *g_lora_b_qkv, *g_lora_a_o, *g_lora_b_o; /* gradient slots (accumulated into) */
  unsigned lora_mask;                   /* bit0 q, bit1 k, bit2 v, bit3 o, bit4 c_fc, bit5 c_proj (lora_a_fc ... below) */
  /* optional 16-bit copies of the four weights and of their transposed copies (clipfs_split_bf16 /
   * clipfs_convert_f16, format in clipfs_tower.weight_format); when present the tower's GEMMs use the
   * bf16 x 3 or f16 MFMA kernel, otherwise the exact fp32 MFMA kernel */
  const void *w_qkv_p, *w_o_p, *w_fc_p, *w_pr_p, *w_qkv_t_p, *w_o_t_p, *w_fc_t_p, *w_pr_t_p;
  /* bias gradient slots (accumulated into by clipfs_tower_bwd / _bwd_sparse; NULL = frozen, nothing launched for it):
   * LayerNorm biases, the q / k / v segments of the packed in-projection bias, out projection, c_fc, c_proj.
   * Refused in the fp16 storage mode (weight_format 2), which keeps dqkv and the MLP gradient as f16 images only. */
  float *g_ln1_b, *g_ln2_b, *g_b_q, *g_b_k, *g_b_v, *g_b_o, *g_b_fc, *g_b_pr;
  /* LoRA on the MLP linears (LinearLoRA.execute, lora_train_vlp.py:296-306, on jclip/model.py:34-39), switched on by
   * lora_mask bit 4 (c_fc: A [r, d], B [4d, r]) and bit 5 (c_proj: A [r, 4d], B [d, r]) with the tower's r / scale / dropout:
   *     u = LN2(x_mid) Wfc^T + b_fc + s * (drop(LN2(x_mid)) A_fc^T) B_fc^T         (u is the saved pre-activation)
   *     x_out = x_mid + g Wpr^T + b_pr + s * (drop(g) A_pr^T) B_pr^T,  g = QuickGELU(u)
   * Dropout streams: dropout_stream0 + 500 + 2 * l (c_fc) and + 1 (c_proj), element (global token row, column).  The g_
   * slots are accumulated into; both NULL = a frozen adapter (only its input-gradient term is computed), exactly one NULL
   * is CLIPFS_EINVAL.  A tower with such an adapter keeps two more [rows, r] tensors per saved record, runs every block on
   * the dense rows (clipfs_tower_pack_mode 0; clipfs_tower_rows_mode 0 when the LAST block has one) and is refused in the
   * fp16 storage mode (h2, g and du exist only as f16 images there), the message naming the block and c_fc / c_proj.
   * Without one, every layout and launch is what it was before these fields existed.  The fields sit in front of the deep
   * prompt's, which stay the tail of the struct; sizeof(clipfs_block) grows either way, so a caller built against the
   * earlier layout is rejected by the block_size check instead of being read at shifted offsets. */
  const float *lora_a_fc, *lora_b_fc, *lora_a_pr, *lora_b_pr;
  float *g_lora_a_fc, *g_lora_b_fc, *g_lora_a_pr, *g_lora_b_pr;
  /* deep prompt (IVLP vision_depth / language_depth, reference jclip/model1.py:95-116): every forward writes `prompt`
   * [prompt_rows, width] over the rows prompt_first ... prompt_first + prompt_rows - 1 of each sequence of the block's
   * input, before LN1 (rows past the sequence -- a trimmed or packed caption -- are skipped: clipfs_prompt_put); every
   * backward takes their gradient right after the block's input gradient exists, accumulates it into g_prompt and zeroes
   * those rows (clipfs_prompt_harvest) -- with g_prompt NULL (a frozen prompt) it only zeroes them.  A block with
   * g_prompt forms its input gradient even as the floor block under stop_at_input.  prompt NULL = no prompt (the fields
   * after it are ignored).  The placement lives here rather than in clipfs_tower so that a tower descriptor keeps its
   * layout; every block of a tower uses the same one (the vision tower's last rows, the text tower's rows 1 ... n). */
  const float* prompt;
  float* g_prompt;
  int prompt_first, prompt_rows;
} clipfs_block;

typedef struct clipfs_tower {
  size_t struct_size;       /* = sizeof(clipfs_tower) of the caller's header (ABI check) */
  size_t block_size;        /* = sizeof(clipfs_block): the stride of `blocks` */
  int width, heads, layers, seq, causal;
  int lora_r;               /* 0 ... 64; ranks above 16 need width % 128 == 0 (the matrix-core adapter kernels) */
  float lora_scale, lora_dropout;
  uint64_t dropout_seed;    /* 0 = no dropout (eval) */
  uint32_t dropout_stream0; /* stream id of layer 0 segment 0; layer l uses stream0 + 4*l + s */
  uint32_t dropout_row0;    /* global index of this call's first token row (data-parallel shards); 0 otherwise */
  const clipfs_block* blocks; /* HOST array [layers] of device pointers */
  int weight_format;        /* format of the blocks' *_p copies: 0 none (exact fp32), 1 bf16 hi/lo, 2 f16 */
  int* gemm_counters;       /* optional: >= clipfs_tower_counter_ints(t, batch) ints, zeroed ONCE by the caller (every
                               GEMM leaves them zero) -- with the scratch enables split-K; one buffer per stream */
  size_t gemm_counters_ints;
  int grad_lo;              /* gradient floor: the lowest block whose parameters train.  0 = every block (today's
                               behaviour).  Blocks below it keep no activations in the forward (same kernels, same
                               dropout masks, same block outputs) and get no backward; their gradient slots must be
                               NULL.  0 <= grad_lo < layers; grad_lo > 0 needs stop_at_input != 0 in the backward
                               (the gradient wrt the tower input runs through every block). */
} clipfs_tower;

/* The two deep-prompt kernels the tower drivers run (also usable alone).  Rows: dense (off == NULL) row(c, j) =
 * c * seq + first + j, skipped when first + j >= seq; packed (off = off[0 .. batch] of a clipfs_tower_bwd_packed plan)
 * row(c, j) = off[c] + first + j, skipped when first + j >= off[c + 1] - off[c] (past the caption's EOT).  j < n, c < batch,
 * every row `width` floats wide.
 *   put:     x[row(c, j), :] = prompt[j, :]
 *   harvest: g[j, :] += sum_c dx[row(c, j), :] (g NULL: nothing added), then those rows of dx -- and of its f16 image dx16
 *            (halves, same layout; NULL = none) -- are set to zero.  Fixed summation order, no atomics: bitwise
 *            reproducible. */
int clipfs_prompt_put(const float* prompt, float* x, const int32_t* off, int batch, int seq, int first, int n, int width,
                      void* stream);
int clipfs_prompt_harvest(float* dx, void* dx16, const int32_t* off, int batch, int seq, int first, int n, int width,
                          float* g, void* stream);

/* floats needed per tower call for saved activations / scratch (saved: one record per block grad_lo ... layers-1;
 * 0 for a descriptor the library rejects) */
size_t clipfs_tower_saved_floats(const clipfs_tower* t, int batch);
size_t clipfs_tower_scratch_floats(const clipfs_tower* t, int batch);
size_t clipfs_tower_counter_ints(const clipfs_tower* t, int batch);
/* x [batch*seq, width] in/out (residual stream, updated in place).  saved == NULL: inference
 * (nothing kept); else activations for clipfs_tower_bwd are written to `saved`. */
int clipfs_tower_fwd(const clipfs_tower* t, float* x, int batch, float* saved, float* scratch, void* stream);
/* The same forward when the caller reads ONE row per sequence of the result (rows[c] = its token index: the class token,
 * jclip/model.py:121-124, or the EOT token, :213-214).  In the LAST block everything after the attention is row-wise,
 * so the output projection, LayerNorm 2 and the MLP run on `batch` rows instead of batch*seq: 9 d^2 MACs per skipped
 * token, 5.9 % of the image tower's forward and 6.0 % of the text tower's at cfg-2.  On return x holds the block output
 * at rows c*seq + rows[c] ONLY (the other rows keep the last block's input); `saved` is complete for
 * clipfs_tower_bwd_sparse with the same rows and NOT for clipfs_tower_bwd.  Falls back to clipfs_tower_fwd in the
 * cases clipfs_tower_bwd_sparse falls back (clipfs_tower_rows_mode() == 0: an o-projection adapter in the last block,
 * seq < 8, CLIPFS_DENSE_BWD=1), so the two always agree.  In the fp16 storage mode the `batch`-row products use the
 * fp32 master weights. */
int clipfs_tower_fwd_rows(const clipfs_tower* t, float* x, const int32_t* rows, int batch, float* saved, float* scratch,
                          void* stream);
int clipfs_tower_rows_mode(const clipfs_tower* t);
/* dx [batch*seq, width] in/out: gradient wrt the tower output on entry, wrt its input on exit.
 * stop_at_input != 0: the gradient wrt the tower input is not needed (image tower without VPT:
 * block 0's LN1 backward and q/k/v dgrad are skipped). */
int clipfs_tower_bwd(const clipfs_tower* t, float* dx, int batch, const float* saved, float* scratch,
                     int stop_at_input, void* stream);
/* The same backward when the gradient wrt the tower output is non-zero in ONE row per sequence only -- which is what
 * both towers receive: the image head reads the class token (jclip/model.py:121-124), the text head the EOT token
 * (:213-214).  dxs [batch, width] holds those rows, rows[b] their token index; dx [batch*seq, width] is written (no
 * zero-filled input needed) with the gradient wrt the tower input.  In the LAST block the MLP and output-projection
 * input-gradients are row-wise, so they run on `batch` rows instead of batch*seq (exact: the skipped rows are exact
 * zeros): 9 d^2 MACs per skipped token, 1.4 % (image) + 1.6 % (text) of the cfg-2 step.  Falls back to the dense path
 * (scatter + clipfs_tower_bwd) for o-projection adapters in the last block and seq < 8 (clipfs_tower_rows_mode). */
int clipfs_tower_bwd_sparse(const clipfs_tower* t, const float* dxs, const int32_t* rows, float* dx, int batch,
                            const float* saved, float* scratch, int stop_at_input, void* stream);
/* The same backward on the LIVE rows of a causal tower (the text tower): below the last block's compact part, the gradient
 * of sequence c is non-zero only on its rows c*seq + 0 .. rows[c] (nothing before the EOT attends to a later row), so
 * every block from the last block's attention down to grad_lo runs its dgrad GEMMs, attention, LayerNorm, LoRA and bias
 * backward on the R = sum (rows[c] + 1) live rows, packed caption after caption (the saved per-row tensors are gathered).
 * plan: int32 device [2 batch + 1 + R] = off[0 .. batch] (exclusive prefix sum of rows[c] + 1, off[batch] = R) |
 * eotp[0 .. batch) (= off[c + 1] - 1) | map[0 .. R) (packed row i -> full-layout row c*seq + i - off[c]); built by the
 * caller from the same rows.  The forward is clipfs_tower_fwd_rows with these rows; dx is written in the full layout
 * (dead rows exact zeros) unless stop_at_input.  Results equal clipfs_tower_bwd_sparse's up to the summation order of the
 * parameter gradients (fewer exact-zero terms).  Runs the dense rows (clipfs_tower_bwd_sparse) when
 * clipfs_tower_pack_mode(t, batch, R) == 0: not causal, the fp16 storage mode, clipfs_tower_rows_mode() == 0, no packed
 * attention kernel for seq, R > batch*seq / 2 (the packed buffers live in the scratch slots of the dense rows: no extra
 * memory), batch*seq < 2048 (launch-bound: nothing to gain), LoRA dropout whose masks are not saved as keep bits (or
 * on an o-projection adapter), or a LoRA / bias workspace the R-row launch would outgrow.  CLIPFS_EINVAL for NULL buffers or R outside [batch, batch*seq]. */
int clipfs_tower_pack_mode(const clipfs_tower* t, int batch, int R);
int clipfs_tower_bwd_packed(const clipfs_tower* t, const float* dxs, const int32_t* rows, const int32_t* plan, int R,
                            float* dx, int batch, const float* saved, float* scratch, int stop_at_input, void* stream);
/* The FORWARD on the live rows (same plan and rows): every block runs its LayerNorms, adapters, GEMMs and attention on the
 * R packed rows, the last block's compact part on the EOT rows; on return x holds the tower output at the rows
 * c*seq + rows[c] (as clipfs_tower_fwd_rows; the other rows of x are unspecified).  Live rows get bitwise the dense
 * forward's values, dropout masks and keep bits included.  `saved` (NULL: no-grad) keeps R rows per block inside the
 * clipfs_tower_saved_floats buffer; its backward is clipfs_tower_bwd_packed_saved.  Runs clipfs_tower_fwd_rows instead
 * (and the backward is then clipfs_tower_bwd_packed) when clipfs_tower_pack_fwd_mode(t, batch, R) == 0: whenever
 * clipfs_tower_pack_mode is 0, outside the exact fp32 mode, where a dense GEMM of the tower's shapes would run split-K
 * at batch*seq rows (an unsplit R-row launch would sum in another order), or with LoRA dropout on an
 * o-projection adapter or on a rank the fused LayerNorm + down-projection does not cover. */
int clipfs_tower_pack_fwd_mode(const clipfs_tower* t, int batch, int R);
int clipfs_tower_fwd_packed(const clipfs_tower* t, float* x, const int32_t* rows, const int32_t* plan, int R, int batch,
                            float* saved, float* scratch, void* stream);
/* clipfs_tower_bwd_packed over the saved tensors of clipfs_tower_fwd_packed (read in place: no gathers).  Same results
 * as clipfs_tower_bwd_packed after clipfs_tower_fwd_rows; CLIPFS_EINVAL where clipfs_tower_pack_fwd_mode is 0. */
int clipfs_tower_bwd_packed_saved(const clipfs_tower* t, const float* dxs, const int32_t* rows, const int32_t* plan, int R,
                                  float* dx, int batch, const float* saved, float* scratch, int stop_at_input, void* stream);

/* ------------------------------------------------------------- cache head --
 * A Tip-Adapter key-value cache over few-shot features with one-hot values (Zhang et al., ECCV 2022), fp32 in every
 * engine precision mode:
 *   a[b,k] = f[b,:] . K[k,:]      E[b,k] = exp(-beta (1 - a[b,k]))      S[b,c] = sum_{k in [off[c], off[c+1])} E[b,k]
 *   logits[b,c] = base[b,c] + alpha S[b,c]
 * f [B, d] query rows (the caller passes unit rows; nothing is normalised or clamped: a > 1 is legal), K [NK, d] keys
 * SORTED BY CLASS, off [C + 1] int32 ascending class offsets into K (off[0] = 0, off[C] = NK; a class may own no key:
 * S = 0), base [B, C] with leading dimension ldbase >= C (NULL: 0), alpha, beta >= 0.  The [B, NK] affinity and E never
 * reach HBM; no float atomics; every sum runs in an order fixed by the shapes and `off` (a class run in ascending key
 * order), every output element is written by one thread: results are bitwise equal run to run.
 *
 * clipfs_cache_plan IS the function the three entry points execute: host-only (no GPU is opened, nothing is launched,
 * nothing written to `plan` on refusal).  CLIPFS_EINVAL, the message naming the argument, for B, NK or C < 1, d not a
 * multiple of 4 in [4, 4096], nA or nB outside [1, 1024] (pass 1 where the operation has no grid), an unknown op or a
 * NULL plan.  The entry points refuse the same before anything is launched, and also: f, K, out or dK NULL or not
 * 16-byte aligned, a leading dimension below C, out == base, alpha or beta negative or not finite. */
#define CLIPFS_CACHE_OP_LOGITS 0 /* clipfs_cache_logits: grid (32-query tiles, chunks of class_chunk classes) */
#define CLIPFS_CACHE_OP_BWD_DK 1 /* clipfs_cache_bwd, the dK launch: grid (32-key tiles, chunks of feat_chunk features) */
#define CLIPFS_CACHE_OP_BWD_DF 2 /*   ... the df launch: grid (32-query tiles, chunks of feat_chunk features) */
#define CLIPFS_CACHE_OP_SEARCH 3 /* clipfs_cache_search: grid (32-query tiles, beta chunks, alpha chunks) */
struct clipfs_cache_plan {
  unsigned grid_x, grid_y, grid_z, block;
  unsigned lds_bytes;     /* static + dynamic LDS of a workgroup (at most 160 KB) */
  int class_chunk;        /* logits: classes per workgroup (0 otherwise) */
  int feat_chunk;         /* backward: features per workgroup, 512, or 128 where 512 would leave compute units idle */
  int beta_chunk;         /* search: betas per workgroup; the affinity is recomputed per chunk (0 otherwise) */
  int alpha_chunk;        /* search: alphas per workgroup (0 otherwise) */
  size_t work_floats;     /* scratch the call needs: 0, no sum is cut over workgroups */
};
int clipfs_cache_plan(int op, int B, int NK, int C, int d, int nA, int nB, struct clipfs_cache_plan* plan);
/* out [B, C] (leading dimension ldout >= C; columns past C and rows past B are not touched) = the logits above, one
 * launch.  out must not alias base. */
int clipfs_cache_logits(const float* f, const float* K, const int32_t* off, const float* base, float* out, int B, int NK,
                        int C, int d, int ldbase, int ldout, float alpha, float beta, void* stream);
/* Backward for key training given dlogits [B, C] (leading dimension lddl >= C), G[b,k] = alpha beta E[b,k] dlogits[b, class(k)]:
 *   dK[k,:] += sum_b G[b,k] f[b,:]   (accumulate-into, like the adapter gradient slots)
 *   df[b,:]  = sum_k G[b,k] K[k,:]   (df may be NULL; written, not accumulated)
 * E is recomputed per 32 x 32 tile; one workgroup owns 32 rows of dK (df) and feat_chunk features and walks the queries (keys)
 * in ascending tiles, so no sum is cut over workgroups: no scratch, one launch per output.  dK and df must not alias
 * f, K or each other.  alpha and beta get no gradient. */
int clipfs_cache_bwd(const float* f, const float* K, const int32_t* off, const float* dlogits, float* dK, float* df, int B,
                     int NK, int C, int d, int lddl, float alpha, float beta, void* stream);
/* The hyper-parameter search in one launch: for the grids alphas [nA], betas [nB] (device, fp32) and targets y [B]
 *   hits[j, i] += #{ b : argmax_c (base[b,c] + alphas[i] S_betas[j][b,c]) == y[b] }        (int32 [nB, nA])
 * ties towards the smaller class index (the rule of clipfs_topk).  Neither the affinity nor S reaches HBM: the keys
 * being class-sorted, classes complete in ascending order along the key walk, and a running (best value, best class)
 * per (query, beta, alpha), updated with a strict > when a class's run ends (with base alone for an empty class), is
 * all that is kept.  Each cell's logits are bitwise those of clipfs_cache_logits.  hits is ADDED to with integer
 * atomics (order-free: deterministic); the caller zeroes it. */
int clipfs_cache_search(const float* f, const float* K, const int32_t* off, const float* base, const int64_t* y,
                        const float* alphas, const float* betas, int32_t* hits, int B, int NK, int C, int d, int ldbase,
                        int nA, int nB, void* stream);

/* ---------------------------------------------------------- TPT objective --
 * The objective of test-time prompt tuning (Shu et al., NeurIPS 2022) for n_img independent images, fp32 in every
 * engine precision mode.  Per image, with F [V, d] the unit view features, T [C, d] the unit class features, s the
 * logit scale:
 *   z_v = s F_v T^T      p_v = softmax(z_v)      H_v = -sum_c p_vc log p_vc
 *   S    = the K views of lowest H_v, ties to the lower view index: rank_v = #{u : H_u < H_v or (H_u == H_v and u < v)},
 *          v in S iff rank_v < K (rank counting, no sort)
 *   pbar = (1/K) sum_{v in S} p_v (ascending view index)      loss = -sum_c pbar_c log pbar_c
 *   dT   = s sum_{v in S} dz_v^T F_v,   dz_v = (1/K) p_v (g - <p_v, g>),   g_c = -log pbar_c
 * (0 log 0 = 0 where pbar underflows).  A view's entropy does not depend on its index: identical rows of F give
 * bitwise equal H, which makes the tie rule exact.  classes == 1 gives loss 0 and a zero gradient.
 *
 * feats [n_img, V, d]; text [C, d], or [n_img, C, d] when text_per_image != 0; selected [n_img, K] int32, ascending
 * view index per image: WRITTEN, or READ when reuse_selection != 0 (the selection is a constant of an episode: later
 * steps reuse the first step's; indices outside [0, V) are clamped); loss [n_img]; entropy [n_img, V] or NULL; dtext
 * [n_img, C, d] = grad_scale * dT or NULL (loss only; grad_scale reaches nothing else); work >=
 * clipfs_tpt_work_floats(n_img, views, width, classes) = n_img * (2 * views * classes + classes) floats.
 *
 * At most three launches whatever n_img (logits tiles on the fp32 matrix cores; one workgroup per image for softmax
 * statistics, entropies, selection, pbar, loss and dz; the rank-K product dz^T F), two when dtext is NULL; nothing is
 * launched per image and nothing returns to the host.  No float atomics: results are bitwise equal run to run, and an
 * image's results do not depend on n_img or on its position in the batch.
 *
 * CLIPFS_EINVAL before anything is enqueued, the message naming the argument: feats, text, selected, loss or work NULL,
 * n_img outside [1, 65535], views outside [1, 1024], width not a multiple of 4 in [4, 1024], classes < 1, K outside
 * [1, views], feats / text / dtext not 16-byte aligned, a scale that is not finite. */
size_t clipfs_tpt_work_floats(int n_img, int views, int width, int classes);
int clipfs_tpt_objective(const float* feats, const float* text, int text_per_image, int32_t* selected, int reuse_selection,
                         int K, float logit_scale, float grad_scale, float* loss, float* entropy, float* dtext, float* work,
                         int n_img, int views, int width, int classes, void* stream);

/* --------------------------------------------------- contrastive objective --
 * The one-directional multi-positive InfoNCE loss (CLIP's contrastive objective with group ids: the UniCL /
 * supervised-contrastive form), fp32 in every engine precision mode.  Both directions of the symmetric loss, and both
 * halves of a data-parallel step, are calls of it.  q [R, d] queries and k [N, d] keys (the caller passes unit rows),
 * q_group [R] / k_group [N] int32, s = logit_scale, w = weight, S = word CLIPFS_SCALER_SCALE of scaler_state (a
 * loss-scaling record, see "loss scaling") or 1 when it is NULL:
 *   z_ij   = s q_i . k_j
 *   a key with k_group[j] < 0 does not exist: it is masked out of the softmax and never positive (padding rows of
 *   gathered blocks); "live" = k_group[j] >= 0
 *   P_i    = { j live : k_group[j] == q_group[i] }      n_i = |P_i|
 *   a row with q_group[i] < 0 or n_i = 0 contributes nothing: loss_i = 0, G_i: = 0; otherwise
 *   loss_i = logsumexp_{j live} z_ij - (1/n_i) sum_{j in P_i} z_ij
 *   loss_rows [R] (may be NULL) = loss_i      loss_sum [1] = w sum_i loss_i
 *   correct [1] (int32, may be NULL) = #{ i : q_group[i] >= 0, n_i > 0, argmax_{j live} z_ij in P_i }, ties to the lower j
 *                                      (the rule of clipfs_topk)
 *   G_ij   = w S (softmax_ij - [j in P_i] / n_i)   for live j, 0 otherwise
 *   dq_i   = s sum_j G_ij k_j   [R, d]             dk_j = s sum_i G_ij q_i   [N, d]
 * dq and dk are each optional (NULL: not formed, one launch fewer).  With its accumulate flag set the finished sum is
 * added ONCE to what is there (bitwise old + fresh); otherwise it is written.  S multiplies the gradients only, never
 * loss_rows, loss_sum or correct.  Plain paired CLIP is group = pair index on both sides.
 *
 * Neither z nor G reaches HBM; no float atomics; every sum runs in an order fixed by (R, N, d), every output element is
 * written by one thread: results are bitwise equal run to run.  Nothing outside the stated extents is touched and
 * nothing returns to the host.  Four launches at most, three when one gradient is NULL:
 *   stats    grid (32-query tiles, chunks of col_chunk keys): per (query, chunk) max, sum of exponentials, sum of
 *            positive z, positive count, best (value, index) into `work`
 *   combine  one workgroup: lse_i, 1 / n_i, loss_i, the hit flag; loss_sum and correct by a fixed-order tree
 *   dq, dk   grid (32 own-row tiles, chunks of feat_chunk features): the other side walked in ascending 32-row tiles,
 *            z recomputed, G formed from lse_i and contracted in the same workgroup
 * work >= work_floats = 6 * chunks * R + 2 * R floats (the same for every op of a shape); no initialisation needed.
 *
 * clipfs_contrastive_plan IS the function the entry point executes: host-only (no GPU is opened, nothing is launched,
 * nothing written to `plan` on refusal).  CLIPFS_EINVAL, the message naming the argument, for R or N < 1, d not a
 * multiple of 4 in [4, 1024], an unknown op or a NULL plan.  clipfs_contrastive_objective refuses the same before
 * anything is enqueued, and also: q, k, q_group, k_group, loss_sum or work NULL; q, k, dq or dk not 16-byte aligned; dq
 * or dk overlapping q, k or each other; a logit_scale or weight that is not finite. */
#define CLIPFS_CONTRASTIVE_OP_STATS 0
#define CLIPFS_CONTRASTIVE_OP_COMBINE 1
#define CLIPFS_CONTRASTIVE_OP_DQ 2
#define CLIPFS_CONTRASTIVE_OP_DK 3
struct clipfs_contrastive_plan {
  unsigned grid_x, grid_y, grid_z, block;
  unsigned lds_bytes;     /* LDS of a workgroup (at most 160 KB) */
  int col_chunk;          /* keys per stats workgroup: a multiple of 128, at most 1024 */
  int chunks;             /* key chunks = ceil(N / col_chunk) */
  int feat_chunk;         /* dq / dk: features per workgroup, 512, or 128 where 512 would leave compute units idle (0 otherwise) */
  size_t work_floats;     /* scratch the call needs */
};
int clipfs_contrastive_plan(int op, int R, int N, int d, struct clipfs_contrastive_plan* plan);
int clipfs_contrastive_objective(const float* q, const float* k, const int32_t* q_group, const int32_t* k_group,
                                 float logit_scale, float weight, const float* scaler_state, float* loss_rows,
                                 float* loss_sum, int32_t* correct, float* dq, int dq_accumulate, float* dk,
                                 int dk_accumulate, float* work, int R, int N, int d, void* stream);

/* ------------------------------------------------------- sigmoid objective --
 * The pairwise sigmoid (SigLIP) loss with group ids, fp32 in every engine precision mode: every (query, key) cell is an
 * independent binary problem, so the loss is one-directional in form and symmetric in effect (one call serves both
 * directions), a batch that repeats classes needs nothing special, and under data parallelism a rank scores ITS
 * queries against all keys.  q [R, d] queries and k [N, d] keys (the caller passes unit rows), q_group [R] / k_group [N]
 * int32, head a DEVICE pointer to two floats (log t, b) -- the scale and bias are trainable, so they never pass
 * through the host --, w = weight, S = word CLIPFS_SCALER_SCALE of scaler_state or 1 when it is NULL:
 *   t = expf(head[0])      a_ij = q_i . k_j      z_ij = t a_ij + head[1]
 *   live(i,j) = q_group[i] >= 0 and k_group[j] >= 0      (a dead cell contributes nothing, anywhere)
 *   pos(i,j)  = live and q_group[i] == k_group[j]
 *   l_ij      = softplus(-z_ij) if pos else softplus(z_ij)      loss_i = sum_j live l_ij
 *   loss_sum [1] = w sum_i loss_i
 *   G_ij      = w S (sigmoid(z_ij) - [pos])   on live cells, 0 elsewhere
 *   dq_i = t sum_j G_ij k_j   [R, d]      dk_j = t sum_i G_ij q_i   [N, d]
 *   dhead [2]: dhead[0] = t sum_ij G_ij a_ij  (d / d log t)      dhead[1] = sum_ij G_ij
 *   correct [1] (int32, may be NULL) = #{ i live with at least one positive : argmax_{j live} z_ij is a positive }, ties
 *                                      to the lower j (the rule of clipfs_topk)
 * UNLIKE the contrastive objective above, a live query WITHOUT a positive still contributes its negative terms to the
 * loss and to every gradient (there, such a row contributes nothing): there is no row normaliser to leave it out of.
 * softplus keeps its tail (max(x, 0) + log1p(exp(-|x|))): at SigLIP's initial point (t, b) = (10, -10) a negative
 * term is 1e-5 ... 1e-7 and there are R N of them; sigmoid does not overflow at any z.
 *
 * dq, dk and dhead are each optional (NULL: not formed).  With its accumulate flag set the finished sum is added ONCE
 * to what is there (bitwise old + fresh); otherwise it is written.  S multiplies the three gradients only.
 *
 * row_stats [4, R] is an OUTPUT, not scratch (the entry point takes none: the gradient kernels need nothing from an
 * earlier pass), and every element of it is written: row 0 loss_i, row 1 sum_j (sigmoid - [pos]), row 2
 * sum_j (sigmoid - [pos]) a_ij (all three 0 for a dead query), row 3 the best live key index as int32 bits, -1 for a
 * dead query or when there is no live key.  The combine kernel reads it, so it must be given.
 *
 * Neither z nor G reaches HBM; no float atomics; every sum runs in an order fixed by (R, N, d), every output element is
 * written by one thread: results are bitwise equal run to run.  Nothing outside the stated extents is touched and
 * nothing returns to the host.  Four launches at most:
 *   rows     grid (32-query tiles): ALL keys walked in tiles of 128, the row statistics into row_stats
 *   combine  one workgroup: loss_sum, correct and dhead from row_stats by a fixed-order tree
 *   dq, dk   grid (32 own-row tiles, chunks of feat_chunk features): the other side walked in ascending 32-row tiles,
 *            z recomputed (the same fp32 number as in the rows kernel), G formed and contracted in the same workgroup
 *
 * clipfs_sigmoid_plan IS the function the entry point executes: host-only (no GPU is opened, nothing is launched,
 * nothing written to `plan` on refusal).  CLIPFS_EINVAL, the message naming the argument, for R or N < 1, d not a
 * multiple of 4 in [4, 1024], an unknown op or a NULL plan.  clipfs_sigmoid_objective refuses the same before anything
 * is enqueued, and also: q, k, q_group, k_group, head, row_stats or loss_sum NULL; q, k, dq or dk not 16-byte aligned;
 * dq or dk overlapping q, k or each other; head overlapping q, k, dq or dk; dhead overlapping q, k, dq, dk or head; a
 * weight that is not finite; a scaler_state that is not 16-byte aligned. */
#define CLIPFS_SIGMOID_OP_ROWS 0
#define CLIPFS_SIGMOID_OP_COMBINE 1
#define CLIPFS_SIGMOID_OP_DQ 2
#define CLIPFS_SIGMOID_OP_DK 3
struct clipfs_sigmoid_plan {
  unsigned grid_x, grid_y, grid_z, block;
  unsigned lds_bytes;     /* LDS of a workgroup (at most 160 KB) */
  int feat_chunk;         /* dq / dk: features per workgroup, 512, or 128 where 512 would leave compute units idle (0 otherwise) */
};
int clipfs_sigmoid_plan(int op, int R, int N, int d, struct clipfs_sigmoid_plan* plan);
int clipfs_sigmoid_objective(const float* q, const float* k, const int32_t* q_group, const int32_t* k_group,
                             const float* head, float weight, const float* scaler_state, float* row_stats,
                             float* loss_sum, int32_t* correct, float* dq, int dq_accumulate, float* dk,
                             int dk_accumulate, float* dhead, int dhead_accumulate, int R, int N, int d, void* stream);

/* --------------------------------------------------- clip pairs objective --
 * CLIP's symmetric pair loss in ONE call with the logit scale on the device: head is a DEVICE pointer to one float,
 * head[0] = log s, so the temperature is trainable and never passes through the host.  With s = expf(head[0]) let
 * C(q, k, qg, kg, s, w) be the contrastive objective above (its live keys, P_i, n_i, dead rows, G and the hit count's
 * ties to the lower index).  S = word CLIPFS_SCALER_SCALE of scaler_state, or 1 when it is NULL:
 *   loss_sum [1] = C(q, k, .., weight_q).loss_sum + C(k, q, .., weight_k).loss_sum
 *   dq [R, d]    = C(q, k).dq + C(k, q).dk            dk [N, d] = C(q, k).dk + C(k, q).dq
 *   correct [2]  (int32, may be NULL) = the hit counts of C(q, k) and C(k, q)
 *   dhead [1]    = sum over both directions of sum_ij G_ij z_ij = d loss / d log s   (S and the weights are inside G)
 * i.e. one G for a cell, with lse_q / n_i the query rows' and lse_k / m_j the key rows' statistics:
 *   G_ij = S (w_q (exp(z_ij - lse_q[i]) - [pos] / n_i) live_k[j] + w_k (exp(z_ij - lse_k[j]) - [pos] / m_j) live_q[i])
 * weight_k == 0 means the second direction DOES NOT EXIST (it is not a multiplication by zero): no key-side statistics
 * are computed, k_stats must be NULL, correct[1] = 0, and the call is C(q, k, .., weight_q) with dhead: the
 * one-directional call a data-parallel rank makes.
 *
 * dq, dk and dhead are each optional (NULL: not formed).  With its accumulate flag set the finished sum is added ONCE
 * to what is there (bitwise old + fresh); otherwise it is written.  S multiplies the three gradients only.
 *
 * q_stats [5, R] and k_stats [5, N] are OUTPUTS, not scratch (the entry point takes none), and every element is
 * written: per row  0 lse,  1 1 / n,  2 the row loss,  3 E_softmax[z] - mean_P z (the row's share of dhead before the
 * weight),  4 the best live index of the other side as int32 bits, -1 for a dead row or when nothing is live.  A row
 * that contributes nothing (dead, or without a positive) has lse = +inf, 1 / n = 0 and rows 2, 3 = 0, which makes its G
 * exactly 0 without a branch.  The gradient launches read rows 0 and 1, the combine launch rows 2 to 4.
 *
 * Neither z nor G reaches HBM; no float atomics; every sum runs in an order fixed by (R, N, d), every output element is
 * written by one thread: results are bitwise equal run to run.  A cell has one fp32 z in every kernel and in both
 * roles.  Nothing outside the stated extents is touched and nothing returns to the host.  Four launches at most:
 *   rows     grid ceil(R / 32) + (both ? ceil(N / 32) : 0): a workgroup walks ALL of the other side in tiles of 128
 *            (no key chunks: their partials would be scratch); the trailing workgroups are the key side
 *   combine  one workgroup: loss_sum, correct and dhead by a fixed-order tree
 *   dq, dk   grid (32 own-row tiles, chunks of feat_chunk features): ONE walk of the other side carries both
 *            directions' G
 *
 * clipfs_clip_pairs_plan IS the function the entry point executes (both = weight_k != 0): host-only.  CLIPFS_EINVAL,
 * the message naming the argument, for R or N < 1, d not a multiple of 4 in [4, 1024], both outside {0, 1}, an unknown
 * op or a NULL plan.  clipfs_clip_pairs_objective refuses the same before anything is enqueued, and also: q, k,
 * q_group, k_group, head, q_stats or loss_sum NULL; k_stats given with weight_k == 0 or NULL with weight_k != 0; q, k,
 * dq or dk not 16-byte aligned; dq or dk overlapping q, k or each other; head, dhead or a statistics array overlapping
 * another array of the call; a weight that is not finite; a scaler_state that is not 16-byte aligned. */
#define CLIPFS_PAIRS_OP_ROWS 0
#define CLIPFS_PAIRS_OP_COMBINE 1
#define CLIPFS_PAIRS_OP_DQ 2
#define CLIPFS_PAIRS_OP_DK 3
struct clipfs_clip_pairs_plan {
  unsigned grid_x, grid_y, grid_z, block;
  unsigned lds_bytes;     /* LDS of a workgroup (at most 160 KB) */
  int feat_chunk;         /* dq / dk: features per workgroup, 512, or 128 where 512 would leave compute units idle (0 otherwise) */
};
int clipfs_clip_pairs_plan(int op, int R, int N, int d, int both, struct clipfs_clip_pairs_plan* plan);
int clipfs_clip_pairs_objective(const float* q, const float* k, const int32_t* q_group, const int32_t* k_group,
                                const float* head, float weight_q, float weight_k, const float* scaler_state,
                                float* q_stats, float* k_stats, float* loss_sum, int32_t* correct, float* dq,
                                int dq_accumulate, float* dk, int dk_accumulate, float* dhead, int dhead_accumulate,
                                int R, int N, int d, void* stream);

/* --------------------------------------------------------------------- TDA --
 * The training-free dynamic adapter (Karmanov et al., "Efficient Test-Time Adaptation of Vision-Language Models",
 * CVPR 2024): a zero-shot classifier adapted at test time by two caches of test features, with no labels, no backward
 * and no extra views; fp32 in every engine precision mode.  The published form handles one image at a time on the
 * host; here one call adapts B samples on the device and IS B applications of the sequential rule in row order.
 *
 * THE RULE.  Fixed: unit class features T [C, d], logit scale s, capacities Sp and Sn (0 disables that cache),
 * pos_alpha, pos_beta, neg_alpha, neg_beta, the entropy band (ent_lo, ent_hi), the mask band (mask_lo, mask_hi).  For
 * one sample with unit feature f at global sample number t:
 *   1. z = s T f      2. lse = logsumexp(z)      3. p_c = exp(z_c - lse)
 *   4. H = -sum_c p_c (z_c - lse) in nats (never the log of an underflowed p; >= 0)
 *   5. pred = argmax z, ties to the lower index (the rule of clipfs_topk)
 *   6. h = H / log2(C) (the published normaliser, although H is in nats; C == 1: h = 0)
 *   7. positive cache, queue of class pred: with fewer than Sp slots occupied take the lowest free slot; otherwise let
 *      w be the occupied slot of largest stored entropy, ties to the most recently inserted, and replace w iff
 *      H < ent[w] (strict, fp32 as stored); else nothing.  An entry is (f, H, t).
 *   8. negative cache, only if ent_lo < h < ent_hi (both strict): the same insertion on the negative queue of class
 *      pred; the entry is (f, H, t, m), m_c = 1 iff mask_lo < p_c < mask_hi.
 *   9. AFTER both updates (a sample sees itself if it was inserted):
 *      out = z + pos_alpha sum_{e in pos} exp(-pos_beta (1 - f . k_e)) onehot(class_e)
 *              - neg_alpha sum_{e in neg} exp(-neg_beta (1 - f . k_e)) m_e
 * update == 0 evaluates step 9 against the state as it stands and changes nothing.  z, H, pred, h and m of a sample
 * are bitwise independent of B and of its row, so the state after any split of a stream into calls is bitwise the
 * same.  At s = 100 confident samples have H near 0 and many comparisons of step 7 are between rounding noise: the
 * fp32 compare and the tie rule make the outcome deterministic all the same.
 *
 * HOW.  Steps 7 and 8 depend only on (pred, H, h) of earlier samples, never on a cache logit, and the queues of
 * different classes are independent.  A scan with one thread per class turns the batch into intervals: entry j (an old
 * slot or a batch row) is in its cache exactly for the batch rows born_j <= i < evict_j, and step 9 is a dense masked
 * sum over (old slots + batch rows).  Five launches at most, whatever B and C: z tiles on the fp32 matrix cores into
 * `out`; per-row statistics; the scan; the masked logits (32 x 32 affinity tiles, contracted on the matrix cores with
 * one-hot class rows or mask rows; the affinity never reaches memory; tiles with no live entry are skipped); the
 * write-back of the survivors (after the logits launch has read the old state; a slot with several occupants within
 * the batch receives the last).  The logits launch is absent when both capacities are 0 (out is then bitwise z), the
 * write-back when update == 0.  No float atomics; every output element is written by one thread.  Summation order of
 * an output element: positive old slots, positive batch rows, negative old slots, negative batch rows, each in
 * ascending tiles of 32 entries, within a tile entries (i, 16 + i) for i = 0 .. 15; then out = z + sum.  Nothing
 * returns to the host.
 *
 * state (all device memory, fixed shapes): pos_keys [C, Sp, d], pos_ent [C, Sp] (+inf = empty), pos_seq [C, Sp] int64
 * (-1 = empty: a slot is occupied iff seq >= 0), the same three for the negative cache, neg_mask [C, Sn, C] bytes,
 * counter [1] int64 = the number of samples seen (t of row b is counter + b; the write-back adds B).  The members of a
 * cache of capacity 0 may be NULL.
 *
 * record: the per-sample OUTPUTS of the call, every element written (none is scratch, none is read before it is
 * written): pred [B] int32, entropy [B] = H, hnorm [B] = h, band [B] int32 (1 iff in the entropy band), seq [B] int64
 * = t, mask [B, C] bytes = m, pos_slot / neg_slot [B] int32 (the slot the sample was inserted into, -1 if it was not),
 * pos_born / pos_evict [C Sp + B] and neg_born / neg_evict [C Sn + B] int32: the interval of old slot (c, k) at index
 * c S + k and of batch row b at index C S + b (born = evict = 0: never in the cache; evict = B: in it when the call
 * ends).
 *
 * out [B, C] with leading dimension ldout >= C; columns past C are not touched.
 *
 * clipfs_tda_plan IS the function the entry point executes: host-only (no GPU is opened, nothing is launched, nothing
 * written to `plan` on refusal).  CLIPFS_EINVAL before anything is enqueued, the message naming the argument: params,
 * state, record or plan NULL or of another struct_size; d not a multiple of 4 in [4, 4096]; C outside [1, 4096]; B
 * outside [1, 8192]; pos_cap or neg_cap outside [0, 8]; an alpha or beta that is negative or not finite; a
 * logit_scale that is not finite; feats, text, out or a key tensor NULL or not 16-byte aligned; ldout below C; a NULL
 * member of record or of an enabled cache; out overlapping feats, text or a key tensor. */
struct clipfs_tda_params {
  unsigned struct_size; /* sizeof(struct clipfs_tda_params) */
  int C, d;
  int pos_cap, neg_cap; /* Sp, Sn */
  float logit_scale;
  float pos_alpha, pos_beta, neg_alpha, neg_beta;
  float ent_lo, ent_hi, mask_lo, mask_hi;
};
struct clipfs_tda_state {
  unsigned struct_size;
  float* pos_keys;
  float* pos_ent;
  int64_t* pos_seq;
  float* neg_keys;
  float* neg_ent;
  int64_t* neg_seq;
  uint8_t* neg_mask;
  int64_t* counter;
};
struct clipfs_tda_record {
  unsigned struct_size;
  int32_t* pred;
  float* entropy;
  float* hnorm;
  int32_t* band;
  int64_t* seq;
  uint8_t* mask;
  int32_t* pos_slot;
  int32_t* neg_slot;
  int32_t* pos_born;
  int32_t* pos_evict;
  int32_t* neg_born;
  int32_t* neg_evict;
};
#define CLIPFS_TDA_LAUNCH_Z 0      /* grid (32-class tiles, 32-row tiles) */
#define CLIPFS_TDA_LAUNCH_STATS 1  /* grid (4-row groups): one wave per row */
#define CLIPFS_TDA_LAUNCH_SCAN 2   /* grid (64-class groups): one thread per class */
#define CLIPFS_TDA_LAUNCH_LOGITS 3 /* grid (32-row tiles, chunks of class_chunk classes) */
#define CLIPFS_TDA_LAUNCH_WRITE 4  /* grid (rows) */
#define CLIPFS_TDA_LAUNCHES 5
struct clipfs_tda_launch {
  unsigned grid_x, grid_y, block, lds_bytes; /* grid_x == 0: the launch is absent */
};
struct clipfs_tda_plan {
  int launches;                 /* launches present: the same for every B and C */
  struct clipfs_tda_launch launch[CLIPFS_TDA_LAUNCHES];
  unsigned lds_bytes;           /* the largest LDS of a workgroup (at most 160 KB) */
  int class_chunk;              /* classes per logits workgroup */
  size_t pos_entries;           /* C Sp + B: elements of pos_born / pos_evict */
  size_t neg_entries;           /* C Sn + B */
  size_t pos_key_floats;        /* C Sp d */
  size_t neg_key_floats;        /* C Sn d */
  size_t neg_mask_bytes;        /* C Sn C */
  size_t mask_bytes;            /* B C: record.mask */
};
int clipfs_tda_plan(const struct clipfs_tda_params* params, int B, int update, struct clipfs_tda_plan* plan);
int clipfs_tda_adapt(const struct clipfs_tda_params* params, const float* feats, const float* text,
                     const struct clipfs_tda_state* state, float* out, int ldout, const struct clipfs_tda_record* record,
                     int B, int update, void* stream);

/* --------------------------------------------------------------- TRANSDUCT --
 * Transductive zero-/few-shot inference (TransCLIP: Zanella, Gerin and Ben Ayed, "Boosting Vision-Language Models with
 * Transduction", NeurIPS 2024): the whole unlabelled test set is classified at once, and its own neighbourhood and
 * cluster structure corrects the zero-shot (or few-shot) predictions.  No labels, no backward, no tower pass; fp32 in
 * every engine precision mode.  Where the published code differs from the rule below, the rule holds.
 *
 * THE RULE.  Inputs: test features F [N, d] (unit rows are assumed, not checked), class features T [C, d], optional
 * labelled shots S [M, d] with labels y [M] (M_c shots of class c; M = 0 is the zero-shot form).  Scalars: logit scale
 * s, neighbours k, init_top m, lam, shot_weight gamma, outer, inner, n_min, var_floor.
 *   1. logy = log_softmax_rows(s F T^T).  The zero-shot label of row i is argmax_c logy_ic, ties to the lower class.
 *   2. nbr_i = the k indices j != i of largest a_ij = f_i . f_j, ties to the lower j (the exclusion is by index: a
 *      duplicate of a feature is a legitimate neighbour), stored in descending a, ties in ascending j, with
 *      w_ir = a_{i, nbr_ir}.  Not symmetrised, not clamped.
 *   3. z = exp(logy); var_d = 1 / d; I_c = the m rows of largest logy_ic (the log-probability, not the probability,
 *      which saturates and ties at s = 100), ties to the lower row, in that order;
 *      mu_c = (sum_{i in I_c} f_i + gamma sum_{y_j = c} s_j) / (m + gamma M_c).
 *   4. `outer` times:
 *      4.1 mu'_c = mu_c / var, b_c = -1/2 sum_d mu_cd mu'_cd, u_ic = lam logy_ic + f_i . mu'_c + b_c.  (Under one
 *          shared diagonal covariance the Gaussian log-likelihood -1/2 sum_d (f_d - mu_cd)^2 / var_d is affine in f up
 *          to a term that does not depend on c, and the softmax removes that term.)
 *      4.2 `inner` times, Jacobi (every row reads the previous sweep's z):
 *          z_i <- softmax_c(u_ic + sum_r w_ir z_{nbr_ir, c}).
 *      4.3 n_c = sum_i z_ic + gamma M_c; G_c = sum_i z_ic f_i + gamma sum_{y_j = c} s_j; mu_c <- G_c / n_c if
 *          n_c > n_min, else mu_c stays.
 *      4.4 var_d <- max(var_floor, (Q_d - 2 sum_c mu_cd G_cd + sum_c n_c mu_cd^2) / (N + gamma M)) with
 *          Q_d = sum_i f_id^2 + gamma sum_j s_jd^2 computed once.
 *   5. Outputs: z, labels_i = argmax_c z_ic (ties low), the zero-shot labels, mu, var, nbr, w.
 *
 * HOW.  Launches of a fit, whatever N, C, d and M: 6 + (knn_chunks > 1) + outer (inner + 4):
 *   logits  s F T^T in 32 x 32 tiles on the fp32 matrix cores into logy
 *   logsm   one wave per row: logy in place, the zero-shot label, z0 = exp(logy)
 *   knn     one workgroup per (32 query rows, column chunk) walks the chunk's key tiles; the N x N similarities never
 *           reach memory; an element's dot is summed in one order wherever it falls, and a row's list is the top k of
 *           a total order (value descending, index ascending), so the result is bitwise independent of the chunking
 *   merge   only with more than one chunk: one thread per row combines the chunks' lists
 *   shots   gamma M_c and gamma sum_{y_j = c} s_j (shots in ascending j); runs (and writes zeros) when M = 0
 *   q       Q_d, in double
 *   init    per class the top m rows of logy (8 row groups, combined in group order), mu, var = 1 / d, mu' = mu / var
 *   per outer iteration:
 *   bias    b_c, one wave per class
 *   u       u = lam logy + F mu'^T + b in the tile kernel of `logits`: lam logy is added HERE, once per outer
 *           iteration, not inside the sweeps; an element is (lam logy + dot) + b
 *   z_step  `inner` launches, one wave per row, the row's t in registers; the sweep reads one z buffer and writes the
 *           other; the last sweep of the fit writes `labels`
 *   stats   G = z^T F on the matrix cores, the rows cut into stat_splits ranges whose partial sums go to stat_work
 *   muvar   combines the partials in range order, then adds the shots' constants; mu, var (its terms summed in double
 *           over 8 class groups combined in group order), mu' for the next iteration
 * bias and muvar are two small launches where one would need a grid-wide barrier (var needs every class, b every
 * feature).  No float atomics; every output element is written by one thread; every sum runs in an order fixed by the
 * shapes; nothing returns to the host; all launches go to `stream`.
 *
 * buffers (all device memory except shot_labels_host; the stages check only the members they use):
 *   inputs   feats [N, d], text [C, d], shots [M, d], shot_labels [M] int32 (both may be NULL when M = 0),
 *            shot_labels_host: an optional HOST copy of the labels, checked for range before anything is enqueued (a
 *            device label outside [0, C) matches no class and cannot send a kernel anywhere)
 *   outputs  z [N, C], labels [N] int32, zs_labels [N] int32, mu [C, d], var [d], nbr [N, k] int32, w [N, k]
 *   state    logy [N, C], u [N, C], z2 [N, C] (the other z buffer), mup [C, d] = mu', bias [C], n [C], G [C, d], Q [d],
 *            shot_n [C], shot_G [C, d], sel [C, m] int32 = I_c
 *   work     stat_work [plan.stat_work_floats], knn_work [plan.knn_work_bytes] (NULL with one chunk)
 * Every element of every state and work buffer is written before it is read.  The O(N C) state is the method's; the
 * workspace of the affinity is knn_work alone: knn_chunks N k 8 bytes.
 *
 * Stages (each runs alone, on the members named): logy (feats, text -> logy, zs_labels, z); knn (feats -> nbr, w);
 * init (feats, logy, shots -> shot_n, shot_G, Q, sel, mu, mup, var); u (feats, logy, mu, mup -> bias, u);
 * z_step (u, nbr, w, z_in -> z_out and, if not NULL, labels); stats (feats, z_in, shot_n, shot_G, Q, mu -> n, G, mu,
 * var, mup).  clipfs_transduct_fit IS these calls in the order of the rule, bit for bit.
 *
 * clipfs_transduct_plan is host-only (no GPU is opened, nothing written to `plan` on refusal).  CLIPFS_EINVAL before
 * anything is enqueued, the message naming the argument: params, buffers or plan NULL or of another struct_size; d not a
 * multiple of 4 in [4, 4096]; C outside [1, 4096]; k outside [1, 8]; init_top outside [1, 16]; N outside
 * [max(k + 1, init_top), 131072]; M outside [0, 65536]; outer or inner below 1; knn_chunks outside [0, 64] (0: the
 * plan decides); logit_scale, lam, shot_weight, n_min or var_floor negative or not finite (var_floor: not positive); a
 * used member NULL or misaligned (16 bytes for the matrices, 4 for the vectors); a written member overlapping another
 * member; a label of shot_labels_host outside [0, C); z_out overlapping z_in, u, nbr or w. */
struct clipfs_transduct_params {
  unsigned struct_size; /* sizeof(struct clipfs_transduct_params) */
  int N, C, d, M;
  int k, init_top, outer, inner;
  int knn_chunks; /* 0: the plan decides; else forced */
  float logit_scale, lam, shot_weight, n_min, var_floor;
};
struct clipfs_transduct_buffers {
  unsigned struct_size;
  const float* feats;
  const float* text;
  const float* shots;
  const int32_t* shot_labels;
  const int32_t* shot_labels_host;
  float* z;
  int32_t* labels;
  int32_t* zs_labels;
  float* mu;
  float* var;
  int32_t* nbr;
  float* w;
  float* logy;
  float* u;
  float* z2;
  float* mup;
  float* bias;
  float* n;
  float* G;
  float* Q;
  float* shot_n;
  float* shot_G;
  int32_t* sel;
  float* stat_work;
  void* knn_work;
};
#define CLIPFS_TRANSDUCT_LAUNCH_LOGITS 0    /* grid (32-class tiles, 32-row tiles) */
#define CLIPFS_TRANSDUCT_LAUNCH_LOGSM 1     /* grid (4-row groups): one wave per row */
#define CLIPFS_TRANSDUCT_LAUNCH_KNN 2       /* grid (32-row tiles, column chunks) */
#define CLIPFS_TRANSDUCT_LAUNCH_KNN_MERGE 3 /* grid (256-row groups); absent with one chunk */
#define CLIPFS_TRANSDUCT_LAUNCH_SHOTS 4     /* grid (classes) */
#define CLIPFS_TRANSDUCT_LAUNCH_Q 5         /* grid (64-feature groups) */
#define CLIPFS_TRANSDUCT_LAUNCH_INIT 6      /* grid (32-class tiles) */
#define CLIPFS_TRANSDUCT_LAUNCH_BIAS 7      /* grid (4-class groups): one wave per class */
#define CLIPFS_TRANSDUCT_LAUNCH_U 8         /* grid (32-class tiles, 32-row tiles) */
#define CLIPFS_TRANSDUCT_LAUNCH_Z_STEP 9    /* grid (4-row groups): one wave per row */
#define CLIPFS_TRANSDUCT_LAUNCH_STATS 10    /* grid (32-class tiles, 128-feature chunks, row ranges) */
#define CLIPFS_TRANSDUCT_LAUNCH_MUVAR 11    /* grid (32-feature groups) */
#define CLIPFS_TRANSDUCT_LAUNCHES 12
struct clipfs_transduct_launch {
  unsigned grid_x, grid_y, grid_z, block, lds_bytes; /* grid_x == 0: the launch is absent */
};
struct clipfs_transduct_plan {
  int launches;    /* of a fit: 6 + (knn_chunks > 1) + outer (inner + 4) */
  int knn_chunks;  /* column chunks of the kNN walk */
  int class_chunk; /* classes a z_step wave holds in registers: 256, 1024 or 4096 */
  int stat_splits; /* row ranges of the stats launch */
  int stat_rows;   /* rows per range (a multiple of 16) */
  struct clipfs_transduct_launch launch[CLIPFS_TRANSDUCT_LAUNCHES];
  unsigned lds_bytes;      /* the largest LDS of a workgroup (at most 160 KB) */
  size_t knn_work_bytes;   /* knn_chunks N k 8, 0 with one chunk */
  size_t stat_work_floats; /* stat_splits C (d + 1) */
  size_t nc_floats;        /* N C: elements of z, z2, logy and u each */
};
int clipfs_transduct_plan(const struct clipfs_transduct_params* params, struct clipfs_transduct_plan* plan);
int clipfs_transduct_logy(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* buffers,
                          void* stream);
int clipfs_transduct_knn(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* buffers,
                         void* stream);
int clipfs_transduct_init(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* buffers,
                          void* stream);
int clipfs_transduct_u(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* buffers,
                       void* stream);
int clipfs_transduct_z_step(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* buffers,
                            const float* z_in, float* z_out, int32_t* labels, void* stream);
int clipfs_transduct_stats(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* buffers,
                           const float* z_in, void* stream);
int clipfs_transduct_fit(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* buffers,
                         void* stream);

/* --------------------------------------------------------------------- SPD --
 * Symmetric positive definite systems in fp32: the blocked Cholesky factor A = L L^T and the solve with many right-hand
 * sides, block 32 on the fp32 matrix cores.  Matrices are row-major with 16-byte-aligned bases; n is a multiple of 4 in
 * [4, 1024]; leading dimensions are multiples of 4 and at least n.  No atomics, no caller memory besides the arguments,
 * nothing returns to the host; results are bitwise equal run to run.
 *
 * clipfs_spd_factor reads ONLY the lower triangle of A (diagonal included) and writes L into the lower triangle of the
 * output and L^T into its strict upper triangle: the whole n x n output is defined (columns n .. ldl of a row are not
 * touched), and the backward substitution reads contiguous rows.  L == A with ldl == lda factors in place (bitwise the
 * out-of-place result); any other overlap is refused.  `info` is a device int32: 0 on success, else the 1-based index of
 * the first pivot that is <= 0 or not finite; the columns before that pivot are valid, later columns are unspecified
 * and may be NaN.  The call always terminates (nothing loops on data) and indexes nothing by a computed value.
 * ceil(n / 32) launches: launch j factors block column j, one workgroup per 32-row tile at or below the diagonal, each
 * forming and factoring the updated diagonal tile itself; diagonal tile j is written by one more workgroup of launch
 * j + 1 (the last one by its own launch), which is what makes the in-place form safe.
 *
 * clipfs_spd_solve: X[i, :] = alpha * A^-1 R[i, :] for the rows i < nrhs (nrhs in [1, 65536]) from the output of
 * clipfs_spd_factor.  X == R with ldx == ldr is allowed; the intermediate of the forward substitution lives in X.  Two
 * launches, forward and backward; one workgroup owns 32 right-hand-side rows, keeps them in LDS (32 (n + 4) floats) and
 * walks the block columns itself.  A factor whose info is not 0 gives unspecified (possibly NaN) values, never a fault.
 *
 * clipfs_spd_plan is host-only (nothing written to `plan` on refusal).  CLIPFS_EINVAL before anything is enqueued, the
 * message naming the argument: n not a multiple of 4 in [4, 1024]; nrhs outside [1, 65536]; a matrix NULL or not
 * 16-byte aligned; lda / ldl / ldr / ldx below n or not a multiple of 4; info NULL or misaligned or inside A or L; L
 * overlapping A, or X overlapping R, other than as the same matrix; X overlapping L; alpha not finite. */
struct clipfs_spd_plan {
  int block;           /* 32 */
  int factor_launches; /* ceil(n / 32) */
  int solve_launches;  /* 2 */
  unsigned factor_grid; /* workgroups of the first factor launch: ceil(n / 32); launch j > 0 has ceil(n / 32) - j + 1 */
  unsigned solve_grid;  /* ceil(nrhs / 32), both launches */
  unsigned threads;     /* 256 */
  unsigned factor_lds_bytes, solve_lds_bytes;
  unsigned lds_bytes;   /* the larger (at most 160 KB) */
};
int clipfs_spd_plan(int n, int nrhs, struct clipfs_spd_plan* plan);
int clipfs_spd_factor(const float* A, int lda, float* L, int ldl, int n, int32_t* info, void* stream);
int clipfs_spd_solve(const float* L, int ldl, int n, const float* R, int ldr, float* X, int ldx, int nrhs, float alpha,
                     void* stream);

/* The panelled pair: the same contract for n a multiple of 4 in [4, 16384], built right-looking over panels of `panel`
 * columns (a multiple of 32 in [32, 1024]) from the kernels above and clipfs_gemm_nt.  WHICH TO CALL: clipfs_spd_factor /
 * clipfs_spd_solve for n <= 1024 (fewer, fused launches; a right-hand side's whole row stays in LDS); the panelled pair
 * above that.  With n <= panel clipfs_spd_factor_panels IS clipfs_spd_factor, launch for launch and bit for bit.
 *
 * clipfs_spd_factor_panels, per panel [c0, c1): (1) the diagonal block by the block-32 factor kernel (ceil(pn / 32)
 * launches, its `info` reports carried to GLOBAL 1-based columns and never overwritten by a later panel: `info` is the
 * FIRST pivot that is <= 0 or not finite); (2) L21 = A21 L11^-T, the forward substitution alone with the rows of A21 as
 * right-hand sides; (3) L21 mirrored into the strict upper triangle; (4) the trailing update A22 -= L21 L21^T in row
 * bands of 4 panels, band b one clipfs_gemm_nt call (alpha = -1, residual = C = the band, sub-matrix views by leading
 * dimension, never split along K) over the columns up to its own last row, so that 1/2 + 2 panel / n of the square's
 * products are formed.  The first panel reads A, every later one L; only the lower triangle of A reaches the result
 * (elements above the diagonal of a band's last block are read and overwritten, their values never used), the whole
 * n x n output is L below and L^T above, L == A with ldl == lda is bitwise the out-of-place result, and columns before a
 * reported pivot are valid.  clipfs_gemm_nt with C == residual (ldc == ldres) is allowed: every element is read and then
 * written by the one thread that owns it.
 *
 * clipfs_spd_solve_panels: X[i, :] = alpha * A^-1 R[i, :].  Forward over the panels: the substitution on the diagonal
 * block (the right-hand sides' panel columns in LDS), then one clipfs_gemm_nt call that takes the panel's part out of
 * all later columns (the panel's rows of L, contiguous); backward from the last panel with the rows of the transposed
 * copy; one last launch scales by alpha.  The right-hand sides live in X (panel 0 reads R), X == R with ldx == ldr is
 * allowed.  This schedule needs no caller scratch, so the call takes none.
 *
 * Launches (clipfs_spd_panels_plan, host-only), P = ceil(n / panel), pn_k = panel k's columns, rest_k = the rows below it:
 *   factor   sum_k ceil(pn_k / 32) + 2 (P - 1) kernel launches and sum_{k < P - 1} ceil(rest_k / (4 panel)) GEMM calls
 *   solve    2 P + 1 kernel launches and 2 (P - 1) GEMM calls
 * No float atomics, nothing returns to the host, results are bitwise equal run to run.  Refusals are those of the pair
 * above with n in [4, 16384], plus: panel not a multiple of 32 in [32, 1024]. */
struct clipfs_spd_panels_plan {
  int panel;           /* as given */
  int panels;          /* P = ceil(n / panel) */
  int band;            /* rows of one trailing-update GEMM call: 4 panel */
  int factor_launches; /* kernel launches of the factor, GEMM calls not counted */
  int factor_gemms;    /* clipfs_gemm_nt calls of the factor */
  int solve_launches;  /* 2 P + 1 */
  int solve_gemms;     /* 2 (P - 1) */
  unsigned threads;    /* 256 */
  unsigned lds_bytes;  /* the largest LDS of a workgroup: the substitution's 32 (min(n, panel) + 4) floats + 25 KB */
};
int clipfs_spd_panels_plan(int n, int nrhs, int panel, struct clipfs_spd_panels_plan* plan);
int clipfs_spd_factor_panels(const float* A, int lda, float* L, int ldl, int n, int panel, int32_t* info, void* stream);
int clipfs_spd_solve_panels(const float* L, int ldl, int n, int panel, const float* R, int ldr, float* X, int ldx, int nrhs,
                            float alpha, void* stream);

/* --------------------------------------------------------------------- GDA --
 * Training-free Gaussian discriminant head (Wang et al., "A Hard-to-Beat Baseline for Training-Free CLIP-Based
 * Adaptation", ICLR 2024): one mean per class and ONE shared full covariance of the few-shot features, shrunk towards
 * its trace; the linear classifier W = Sigma^-1 mu is added to the zero-shot logits with one weight alpha.  No training,
 * no backward, no tower pass; fp32.  Where the published code differs from the rule below, the rule holds.
 *
 * THE RULE.  Inputs: shots S [M, d] with unit rows (assumed, not checked), SORTED BY CLASS; offsets int32 [C + 1]
 * (class c owns rows offsets[c] .. offsets[c + 1] - 1); every class owns at least one shot and M >= 2.  d is a multiple
 * of 4 in [4, 1024], C in [1, 4096], M in [2, 65536].
 *   1. mu_c = the mean of class c's shots: an fp32 sum in row order divided by n_c.
 *   2. X = S - mu_y, stored transposed as xt [d, Mp], Mp = M rounded up to 32, the tail zero.
 *   3. G = xt xt^T [d, d]: one clipfs_gemm_nt call (K = Mp takes its K % 32 == 0 path).
 *   4. tau = trace(G), summed in double in a fixed order; A = G + shrink tau / (M - 1) I (shrink >= 0, 1 by default).
 *      With Sigma = G / (M - 1) this is the published (M - 1) Sigma + trace(Sigma) I.  No host synchronisation: with
 *      tau = 0 (or shrink = 0 and a singular G) A is singular and `info` reports it.
 *   5. A = L L^T (clipfs_spd_factor), Z = A^-1 mu with rows as right-hand sides, W = d Z [C, d] (clipfs_spd_solve with
 *      alpha = d).
 *   6. b_c = log pi_c - 1/2 mu_c . W_c; pi_c = 1 / C (CLIPFS_GDA_PRIOR_UNIFORM) or n_c / M (_EMPIRICAL).
 *   7. logits = base + alpha (F W^T + b) for unit test features F [B, d] and the caller's zero-shot logits base [B, C]
 *      (NULL: 0): ONE clipfs_gemm_nt call with alpha, bias = alpha b and residual = base; there is no kernel for it here.
 *   8. The alpha search runs on g = F W^T + b, formed once: hits[a] = the number of rows whose
 *      argmax_c (base + alphas[a] g) equals the target, the argmax taking the lowest index on ties; all nA in [1, 1024]
 *      cells in one launch.
 *
 * buffers (device memory except offsets_host).  Every intermediate is a named output, written whole before it is read:
 *   inputs   shots [M, d], offsets [C + 1] int32, offsets_host: an optional HOST copy of the offsets, checked before
 *            anything is enqueued (a device copy that disagrees cannot send a kernel anywhere: the kernels clamp it)
 *   outputs  mu [C, d], xt [d, Mp], gram [d, d] (G after step 3, A after step 4), tau [1], chol [d, d] (L below and on
 *            the diagonal, L^T above), info [1] int32 (clipfs_spd_factor's), W [C, d], b [C]
 * Stages (each runs alone on the members named): stats (shots, offsets -> mu, xt); shrink (gram -> gram, tau);
 * bias (mu, W, offsets -> b).  clipfs_gda_fit IS stats, clipfs_gemm_nt (xt -> gram, without a split-K workspace), shrink,
 * clipfs_spd_factor (gram -> chol, info), clipfs_spd_solve (chol, mu -> W) and bias in this order on `stream`, bit for
 * bit: 6 + ceil(d / 32) launches, a function of d alone, no host synchronisation, no float atomics.
 *
 * clipfs_gda_search(g [B, C], base [B, C] with row stride ldbase or NULL, target int64 [B], alphas [nA], hits int32
 * [nA]): zeroes `hits` on the stream, then one launch; rows are counted in LDS integers and added with integer atomics.
 *
 * clipfs_gda_plan is host-only (nothing written to `plan` on refusal).  CLIPFS_EINVAL before anything is enqueued, the
 * message naming the argument: params, buffers or plan NULL or of another struct_size; d not a multiple of 4 in
 * [4, 1024]; C outside [1, 4096]; M outside [2, 65536] or below C; prior unknown; shrink negative or not finite; a used
 * member NULL or misaligned (16 bytes for the matrices, 4 for the vectors); a written member overlapping another
 * member; in offsets_host: offsets[0] != 0, a class without a shot, a descending entry, offsets[C] != M; in the search:
 * B, C or nA out of range, a NULL or misaligned argument, ldbase below C. */
#define CLIPFS_GDA_PRIOR_UNIFORM 0
#define CLIPFS_GDA_PRIOR_EMPIRICAL 1
struct clipfs_gda_params {
  unsigned struct_size; /* sizeof(struct clipfs_gda_params) */
  int M, C, d;
  int prior;    /* CLIPFS_GDA_PRIOR_* */
  float shrink; /* 1: the published rule */
};
struct clipfs_gda_buffers {
  unsigned struct_size;
  const float* shots;
  const int32_t* offsets;
  const int32_t* offsets_host;
  float* mu;
  float* xt;
  float* gram;
  float* tau;
  float* chol;
  int32_t* info;
  float* W;
  float* b;
};
struct clipfs_gda_plan {
  int launches;        /* of a fit: 6 + ceil(d / 32) */
  int Mp;              /* M rounded up to 32: the row length of xt */
  int factor_launches; /* ceil(d / 32) */
  int solve_launches;  /* 2 */
  unsigned stats_grid, bias_grid, solve_grid, threads;
  unsigned lds_bytes; /* the largest LDS of a workgroup (the solve's; at most 160 KB) */
  size_t xt_floats;   /* d Mp */
};
int clipfs_gda_plan(const struct clipfs_gda_params* params, struct clipfs_gda_plan* plan);
int clipfs_gda_stats(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* buffers, void* stream);
int clipfs_gda_shrink(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* buffers, void* stream);
int clipfs_gda_bias(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* buffers, void* stream);
int clipfs_gda_search(const float* g, const float* base, int ldbase, const int64_t* target, const float* alphas,
                      int32_t* hits, int B, int C, int nA, void* stream);
int clipfs_gda_fit(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* buffers, void* stream);

/* --------------------------------------------------------------------- KRR --
 * Kernel ridge regression head (ProKeR: Bendou et al., "ProKeR: A Kernel Perspective on Few-Shot Adaptation of Large
 * Vision-Language Models", CVPR 2025): the Tip-Adapter kernel k(x, s) = exp(-beta (1 - x . s)) with the global closed-form
 * solution of the ridge problem in its RKHS, regularised towards a base predictor.  Training-free, fp32, no backward.
 * More general than the paper in two places: the base predictor is whatever logits the caller supplies (for the shots
 * and for the queries; NULL: 0), and the one-hot targets carry a scale t.
 *
 * THE RULE.  Inputs: shots S [n, d] with unit rows (assumed, not checked) in ANY label order, labels int32 [n], base_S
 * [n, C] (row stride ldbs) or NULL.  d a multiple of 4 in [4, 1024], n in [1, 16384], C in [1, 4096], beta in (0, 100],
 * lambda > 0 and finite, t finite.  n4 = 4 ceil(n / 4).
 *   1. A [n4, n4] = exp(-beta (1 - S S^T)) + lambda I: one clipfs_gemm_nt call (S S^T into A) and one map launch in
 *      place, exp as exp2((a - 1) (beta log2 e)), the diagonal computed like any other element, then + lambda.  Pad rows
 *      and columns (n .. n4) are the identity, written by the map; the whole n4 x n4 matrix is defined.
 *   2. Et [C, n4]: Et[c, j] = t [labels[j] == c] - base_S[j, c]; pad columns are 0.  One class per row: the layout the
 *      solves take as right-hand sides.  A label outside [0, C) matches no class (labels are compared, never used as an
 *      index); labels_host, an optional HOST copy, is checked before anything is enqueued.
 *   3. A = L L^T and At = Et A^-1 (rows as right-hand sides): clipfs_spd_factor / clipfs_spd_solve when n4 <= 1024, the
 *      panelled pair with `panel` above that.  At [C, n4] has the contraction index contiguous; its pad columns are 0.
 *   4. out[b, c] = base[b, c] + sum_{j < n} exp(-beta (1 - x_b . s_j)) At[c, j] for queries X [B, d] (clipfs_krr_apply).
 *
 * clipfs_krr_apply: one workgroup per 32 query rows and class chunk, grid (ceil(B / 32), ceil(C / class_chunk)).  It walks
 * the keys in tiles of 32: both operands pass through LDS, the four waves' partial dot products are added in wave order,
 * g is formed once in LDS, then every wave contracts g with the rows of At for its share of the 32-class tiles on
 * v_mfma_f32_32x32x2_f32, the accumulators in registers: tiles_per_wave in {1, 2, 4, 8}, class_chunk = 128 tiles_per_wave
 * (1024 classes at 8; more classes go over grid.y, each chunk forming g again).  The [B, n] affinity never reaches memory;
 * no float atomics; a row's result depends on neither B nor the other rows; bitwise equal run to run.  base (NULL: 0) and
 * out are [B, C] with row strides ldbase, ldo (column slices); out must not overlap base.
 *
 * clipfs_krr_fit IS clipfs_krr_system, clipfs_krr_targets, the factor and the solve in this order on `stream`, bit for
 * bit; every intermediate is a named output.  buffers: inputs shots, labels, labels_host (host, optional), base_S + ldbs
 * (optional); outputs A [n4, n4], chol [n4, n4] (may be A: the factor runs in place), info [1] int32, Et [C, n4], At
 * [C, n4] (may be Et); there is no caller scratch.  Launches: 3 (one of them the GEMM call) + the
 * factor's + the solve's, a closed form of (n, panel) that clipfs_krr_plan returns.
 *
 * clipfs_krr_plan(n, C, d, B, panel) is host-only (nothing written on refusal).  CLIPFS_EINVAL before anything is
 * enqueued, the message naming the argument: d, n, C, B, panel, beta, lambda, t out of range; ld / ldet / ldat / ldbs /
 * ldbase / ldo too small (or, for A, Et and At, not a multiple of 4); a pointer NULL or misaligned (16 bytes for the
 * matrices, 4 for labels and info); out overlapping base; a label of labels_host outside [0, C); params or buffers NULL
 * or of another struct_size; a written member of the fit overlapping another member (other than chol == A, At == Et). */
struct clipfs_krr_params {
  unsigned struct_size; /* sizeof(struct clipfs_krr_params) */
  int n, C, d;
  int panel;    /* of the panelled factor and solve (used when n4 > 1024) */
  float beta;   /* kernel sharpness */
  float lambda; /* ridge */
  float t;      /* target scale */
};
struct clipfs_krr_buffers {
  unsigned struct_size;
  const float* shots;
  const int32_t* labels;
  const int32_t* labels_host;
  const float* base_S;
  int ldbs;
  float* A;
  float* chol;
  int32_t* info;
  float* Et;
  float* At;
};
struct clipfs_krr_plan {
  int n4;              /* 4 ceil(n / 4) */
  int panelled;        /* 1: n4 > 1024, the panelled factor and solve */
  int fit_launches;    /* kernel launches and GEMM calls of a fit */
  int factor_launches; /* of these: the factor's ... */
  int solve_launches;  /* ... and the solve's (GEMM calls included) */
  int tiles_per_wave;  /* of the apply: 32-class accumulators per wave */
  int class_chunk;     /* 128 tiles_per_wave */
  unsigned apply_grid_x, apply_grid_y, threads;
  unsigned lds_bytes;  /* the largest LDS of a workgroup (at most 160 KB) */
};
int clipfs_krr_plan(int n, int C, int d, int B, int panel, struct clipfs_krr_plan* plan);
int clipfs_krr_system(const float* S, float* A, int n, int d, int ld, float beta, float lambda, void* stream);
int clipfs_krr_targets(const int32_t* labels, const int32_t* labels_host, const float* base_S, int ldbs, float* Et, int n, int C,
                       int ldet, float t, void* stream);
int clipfs_krr_apply(const float* X, const float* S, const float* At, int ldat, const float* base, int ldbase, float* out,
                     int ldo, int B, int n, int C, int d, float beta, void* stream);
int clipfs_krr_fit(const struct clipfs_krr_params* params, const struct clipfs_krr_buffers* buffers, void* stream);

/* ------------------------------------------------------------- OT matching --
 * Optimal-transport matching of M local image features against the N prompt features of every class (PLOT: Chen et al.,
 * "Prompt Learning with Optimal Transport for Vision-Language Models", ICLR 2023), fp32 in every precision mode.  The
 * [B, C, M, N] similarity never reaches memory.  Where the published code differs from the rule below, the rule holds.
 *
 * THE RULE.  Inputs: X [B, M, d] and P [C, N, d], fp32 rows that the caller has normalised to unit length (assumed, not
 * checked); marginals mu [B, M] and nu [C, N], positive, each row summing to 1 (NULL: uniform 1/M, 1/N); eps, iters,
 * scale.
 *   z[b,c,m,n] = X[b,m,:] . P[c,n,:]
 *   K = exp((z - 1) / eps)                       (exp2((z - 1) * (log2e / eps)) on the device)
 *   v = 1
 *   repeat iters times:   u = mu / (K v)      v = nu / (K^T u)      (this order)
 *   T = diag(u) K diag(v)
 *   logits[b,c] = scale * sum_{m,n} T z
 * Backward: T is a constant, as in PLOT (its Sinkhorn runs under no_grad).  With G = dlogits[b,c] * scale * T[b,c,m,n]:
 *   dP[c,n,:] = sum_{b,m} G X[b,m,:]             dX[b,m,:] = sum_{c,n} G P[c,n,:]
 *
 * DEVIATION FROM THE PAPER.  `iters` is fixed (100 in PLOT's configuration).  PLOT stops early once the batch mean of
 * |u - u_prev| falls below 1e-2: a loop whose length depends on the data, decided by a host read.  It is not offered.
 *
 * Limits: d a multiple of 4 in [4, 1024]; M in [1, 256]; N in [1, 32]; eps in [0.05, 10]; iters in [1, 1000]; scale
 * finite; B and C in [1, 2^20] with B M <= 2^24, C N <= 2^24 and B C <= 2^28.  The lower eps bound is derived: with unit
 * rows z >= -1, so K >= exp(-2 / eps) = exp(-40) = 4e-18 at eps = 0.05 and u, v and T stay finite in fp32; at
 * eps = 0.02 K reaches exp(-100), which is subnormal.
 *
 * clipfs_ot_logits (replaces PLOT's `sim = einsum('mbd,ncd->mnbc')`, `Sinkhorn(KK, u, v)` and
 * `sim_op = sum(T * sim, dim=(0, 1))`): ONE launch.  Outputs logits [B, C] (row stride ldl >= C; the columns past C are
 * not touched), u [B, C, M] and v [B, C, N]: the scalings after the last iteration, which clipfs_ot_bwd reads.  There is
 * no caller scratch.  One workgroup owns an image and a chunk of classes, forms the chunk's z on the fp32 matrix cores
 * into LDS, and each wave then iterates one class at a time with K in registers.
 *
 * clipfs_ot_bwd (replaces autograd through `sum(T * sim)` with T detached): one launch for dP [C, N, d] and, with dX
 * not NULL, one for dX [B, M, d], both walks of 32 x 32 tiles that form z again (the same fp32 number per cell as the
 * forward held) and G from u, v and dlogits [B, C] (row stride ldd >= C).  accumulate != 0 adds to dP / dX.
 *
 * No float atomics; every output element is written by one thread; the order of every sum depends on the shapes alone;
 * nothing returns to the host; results are bitwise equal run to run, and a (b, c) cell does not depend on which other
 * images and classes share the call.  A forward workgroup that needs more than 64 KB of LDS (M > 224) asks for it.
 *
 * clipfs_ot_plan is host-only (nothing written to `plan` on refusal).  CLIPFS_EINVAL before anything is enqueued, the
 * message naming the argument: a shape, eps, iters or scale outside the limits; ldl or ldd below C; X, P, logits, u, v,
 * dlogits or dP NULL; X, P, dP or dX not 16-byte aligned (the others: 4); an output overlapping an input or another
 * output. */
struct clipfs_ot_plan {
  int fwd_launches, dp_launches, dx_launches; /* 1, 1, 1 */
  int rows_per_lane; /* rows of z a lane of the forward owns: ceil(M / 64) rounded up to 1, 2 or 4 */
  int prompt_regs;   /* N rounded up to 4, 8, 16 or 32: the forward instantiation */
  int class_chunk;   /* classes per forward workgroup */
  int class_chunks;  /* ceil(C / class_chunk) */
  int z_stride;      /* row stride of z in LDS: 32 ceil(class_chunk N / 32) + 1 */
  int dp_feat_chunk, dx_feat_chunk; /* features per gradient workgroup: 512 or 128 */
  unsigned fwd_grid; /* B class_chunks */
  unsigned dp_grid_x, dp_grid_y; /* (ceil(C N / 32), ceil(d / dp_feat_chunk)) */
  unsigned dx_grid_x, dx_grid_y; /* (ceil(B M / 32), ceil(d / dx_feat_chunk)) */
  unsigned threads;  /* 256 */
  unsigned fwd_lds_bytes; /* 4 * 32 ceil(M / 32) * z_stride (at most 66 560) */
  unsigned bwd_lds_bytes;
};
int clipfs_ot_plan(int B, int M, int C, int N, int d, struct clipfs_ot_plan* plan);
int clipfs_ot_logits(const float* X, const float* P, const float* mu, const float* nu, float* logits, int ldl, float* u,
                     float* v, int B, int M, int C, int N, int d, float eps, int iters, float scale, void* stream);
int clipfs_ot_bwd(const float* X, const float* P, const float* u, const float* v, const float* dlogits, int ldd, float* dP,
                  float* dX, int B, int M, int C, int N, int d, float eps, float scale, int accumulate, void* stream);

/* ------------------------------------------------------------------ AUGMIX --
 * AugMix test-time views (Hendrycks et al., "AugMix: A Simple Data Processing Method to Improve Robustness and
 * Uncertainty", ICLR 2020; the views test-time prompt tuning and TDA are published with) generated on the device from the
 * uint8 image pool of clipfs_crop_batch, every uint8 image equal to PIL's bit for bit.  The host samples the recipe, the
 * device does the pixels.  Where the published AugMix or TPT code differs from the rule below, the rule holds.
 *
 * THE RULE.  S is the view side.  `base` is the S x S x 3 uint8 image of the view's crop record: its arithmetic and its
 * record {src, top, left, h, w, flip, out_w, out_h, win_x, win_y, filter, 0} are exactly those of clipfs_crop_batch.  A
 * view has `width` chains; chain i starts from base and applies depth[i] operations, 0 to 3 of them, each reading a whole
 * uint8 image and writing a whole uint8 image.  A chain of depth 0 is base itself.  Operations {code, param}:
 *   NONE (0)          copy.
 *   AUTOCONTRAST (1)  per channel (ImageOps.autocontrast, cutoff 0): lo and hi are the lowest and highest occupied bins of
 *                     the channel's histogram.  hi <= lo: the LUT is the identity.  Otherwise in double, every operation
 *                     rounded on its own: scale = 255.0 / (hi - lo), offset = -lo * scale,
 *                     lut[i] = clamp(int(i * scale + offset), 0, 255), int() towards zero.
 *   EQUALIZE (2)      per channel (ImageOps.equalize), all in integers: h the histogram,
 *                     step = (sum(h) - (last non-zero entry of h)) / 255.  At most one occupied bin, or step == 0: the
 *                     LUT is the identity.  Otherwise n = step / 2; for i = 0 .. 255: lut[i] = min(n / step, 255), then
 *                     n += h[i] (the clamp is Image.point's).
 *   POSTERIZE (3)     param = bits in [1, 8]: v & ~((1 << (8 - bits)) - 1).
 *   SOLARIZE (4)      param = threshold in [0, 256]: v < threshold ? v : 255 - v.
 *   AFFINE (5)        six double coefficients a0 .. a5 (Image.transform((S, S), AFFINE, a, BILINEAR)), fill 0.  For output
 *                     pixel (x, y), in double, every multiply and add rounded on its own (no fma):
 *                       xin = a0 (x + 0.5) + a1 (y + 0.5) + a2;  yin = a3 (x + 0.5) + a4 (y + 0.5) + a5  (left to right)
 *                       xin < 0 || xin >= S || yin < 0 || yin >= S: the pixel is 0 in all channels.  Otherwise
 *                       xin -= 0.5; yin -= 0.5; X = floor(xin); Y = floor(yin); dx = xin - X; dy = yin - Y
 *                       x0 = clamp(X, 0, S-1), x1 = clamp(X+1, 0, S-1), yc = clamp(Y, 0, S-1)
 *                       v1 = in[yc][x0] + (in[yc][x1] - in[yc][x0]) * dx
 *                       v2 = the same on row Y + 1 if 0 <= Y + 1 < S, else v1
 *                       out = (uint8)(v1 + (v2 - v1) * dy), truncated.
 * The output view, in fp32, every operation rounded on its own:  t(u) = (u8 - mean * 255) * ((1 / 255) / std), the formula
 * of clipfs_crop_batch;  acc = 0;  for i ascending: acc = acc + w[i] * t(chain_i);
 *   out = m * t(base) + (1 - m) * acc,   fp32 [n, 3, S, S].
 * With m = 1 and all depths 0 this is bitwise clipfs_crop_batch's out_norm for the same record.
 *
 * clipfs_augmix_batch: pool, source table and crop records as clipfs_crop_batch takes them (host tables validated, device
 * copies read and re-checked by the kernels, which write nothing for a view that fails).  The recipe tables, each as a HOST
 * copy (validated before anything is enqueued) and a device copy (read by the kernels, which execute no chain the host
 * would have refused): ops int32 [n, width, 3, 2] = {code, param}; coef float64 [n, width, 3, 6] (read for AFFINE steps
 * only); depth int32 [n, width]; w fp32 [n, width]; m fp32 [n].  Entries of ops and coef at or past a chain's depth are
 * ignored.  mean, std: device fp32 [3].  base_u8 [n, S, S, 3] and chains_u8 [n, width, S, S, 3] are caller-owned uint8
 * device buffers, documented OUTPUTS and the only working storage: base_u8 is the crop, chains_u8[v, i] the final image of
 * chain i (base for depth 0).  Every element of base_u8, chains_u8 and out is written, none is read before it is
 * written; there is no hidden scratch and no host synchronisation.
 *
 * Three launches on `stream`: base (the crop; grid (n, ceil(S / 16)), the resampling of crop_batch_kernel), chains (one
 * workgroup of 1024 threads per (view, chain), the image resident in LDS for the whole chain: integer LDS histogram, LUT,
 * in-place apply; AFFINE reads LDS, writes chains_u8 and reads it back if another operation follows), mix (four pixels per
 * thread).  No float atomics; every output element is written by one thread; results are bitwise equal run to run, and a
 * view's result does not depend on what shares the call.
 *
 * Limits: S in [8, 224] (one view's image, 150 528 bytes at S = 224, with its histograms and LUTs, is one CU's LDS; the
 * 336-px towers are not offered), width in [1, 4], n in [1, 65 536], sources as clipfs_crop_batch.
 *
 * clipfs_augmix_plan(n, S, width) is host-only (no GPU is opened, nothing written on refusal) and IS the function the
 * entry point executes: the three launches and the byte sizes of the two uint8 buffers.  The base launch's lds_bytes is its
 * bound at 80 taps; a call asks for what its batch's largest tap count needs.  CLIPFS_EINVAL before anything is enqueued,
 * the message naming the argument: n, S or width out of range; a NULL or misaligned pointer (base_u8, chains_u8 and out:
 * 16 bytes; coef and the source table: 8; the other tables: 4); an op code outside 0..5; bits or threshold out of range; a
 * depth outside 0..3; a non-finite coefficient, weight or m; everything clipfs_crop_batch refuses about a source or a
 * record; out, base_u8 and chains_u8 overlapping each other or the pool; recipe NULL or of another struct_size. */
enum { CLIPFS_AUGMIX_LAUNCH_BASE = 0, CLIPFS_AUGMIX_LAUNCH_CHAINS = 1, CLIPFS_AUGMIX_LAUNCH_MIX = 2 };
enum {
  CLIPFS_AUGMIX_NONE = 0, CLIPFS_AUGMIX_AUTOCONTRAST = 1, CLIPFS_AUGMIX_EQUALIZE = 2, CLIPFS_AUGMIX_POSTERIZE = 3,
  CLIPFS_AUGMIX_SOLARIZE = 4, CLIPFS_AUGMIX_AFFINE = 5
};
struct clipfs_augmix_recipe {
  unsigned struct_size; /* sizeof(struct clipfs_augmix_recipe) */
  const int32_t *ops, *ops_dev;
  const double *coef, *coef_dev;
  const int32_t *depth, *depth_dev;
  const float *w, *w_dev;
  const float *m, *m_dev;
};
struct clipfs_augmix_launch {
  unsigned grid_x, grid_y, block, lds_bytes;
};
struct clipfs_augmix_plan {
  int launches;                          /* 3 */
  struct clipfs_augmix_launch launch[3]; /* by CLIPFS_AUGMIX_LAUNCH_* */
  unsigned lds_bytes;                    /* of a chain workgroup, the largest (at most 160 KB) */
  size_t base_bytes;                     /* n S S 3 */
  size_t chains_bytes;                   /* n width S S 3 */
  size_t out_floats;                     /* n 3 S S */
};
int clipfs_augmix_plan(int n, int S, int width, struct clipfs_augmix_plan* plan);
int clipfs_augmix_batch(const uint8_t* pool, size_t pool_bytes, const int64_t* src, const int64_t* src_dev, int n_src,
                        const int32_t* recs, const int32_t* recs_dev, int n, int S, int width,
                        const struct clipfs_augmix_recipe* recipe, const float* mean, const float* stdv, uint8_t* base_u8,
                        uint8_t* chains_u8, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIPFS_H */
