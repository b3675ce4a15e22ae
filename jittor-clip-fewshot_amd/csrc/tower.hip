// Host-side sequencing of one transformer tower (forward and backward): the C++ runtime that replaces
// Jittor's graph executor for Transformer / ResidualAttentionBlock (jclip/model.py:42-77),
// PlainMultiheadAttentionLoRA (lora_train_vlp.py:431-506) and their autograd.  One call enqueues
// every kernel of the pass on the caller's stream; no allocation, no synchronisation.
//
// Residual stream without copies: block l reads x_in[l], the out-projection epilogue writes
// x_mid[l] = x_in[l] + attn, the c_proj epilogue writes x_in[l+1] = x_mid[l] + mlp, so the tensors the
// backward needs are exactly the ones the forward had to produce anyway.
//
// The transformer block is written once per direction (fwd_block; bwd_mlp_half + bwd_attn_half).  A RowView says which
// rows a walk runs on -- every row, or the live rows of a causal tower's plan -- and each step picks its kernel variant
// from the view where the step is written.  The last block's one-row-per-sequence part is fwd_tail / bwd_head.
#include "common.h"

#include <stdlib.h>

// the GEMM helper's arguments are named at the call site: designated initialisers, which clang accepts under -std=c++17
#pragma clang diagnostic ignored "-Wc++20-designator"

namespace clipfs {

static inline size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }

// fp16 storage mode runs attention on the f16 MFMA kernels (attention_f16.hip; sequences up to its bound, 1024 tokens)
static inline bool f16_attention(const clipfs_tower* t) {
  return t->weight_format == 2 && t->seq <= clipfs_attention_f16_max_seq();
}
// ... and then qkv itself is stored as f16 (written by the QKV GEMM, read by the attention kernels): needs the
// f16 x f16 GEMM for the LoRA'd projection, i.e. a segment width that is a multiple of its 128-column tiles
static inline bool qkv_f16(const clipfs_tower* t) {
  return f16_attention(t) && (t->width % 128) == 0 && t->lora_r <= 64;
}

// which adapters of a block are switched on (clipfs_block.lora_mask: bits 0..2 = q / k / v, bit 3 = the out-projection,
// bit 4 = mlp.c_fc, bit 5 = mlp.c_proj)
struct Adapters {
  unsigned qkv_mask;
  bool o, fc, pr;
  bool mlp() const { return fc || pr; }
};
static inline Adapters adapters(const clipfs_block& b) {
  return {b.lora_a_qkv ? (b.lora_mask & 7u) : 0u, b.lora_a_o && (b.lora_mask & 8u), b.lora_a_fc && (b.lora_mask & 16u),
          b.lora_a_pr && (b.lora_mask & 32u)};
}
// some block of the tower has an MLP adapter: the saved record gets the t_fc | t_pr slot, the adapter workspace covers the
// rectangular products, and every walk keeps the dense rows.  Without one nothing of the layouts or launches changes.
static bool tower_has_mlp_lora(const clipfs_tower* t) {
  if (!t->blocks || t->block_size != sizeof(clipfs_block) || t->lora_r <= 0) return false;
  for (int l = 0; l < t->layers; ++l)
    if (adapters(t->blocks[l]).mlp()) return true;
  return false;
}
// dropout streams of block l's MLP adapters (c_fc, then c_proj): disjoint from the attention adapters' stream0 + 4 l + s
static inline uint32_t mlp_stream(const clipfs_tower* t, int l) { return t->dropout_stream0 + 500u + 2u * (uint32_t)l; }

struct SavedLayout {
  size_t x_in, stat1, h1, t_qkv, qkv, att, lse, t_o, x_mid, stat2, u, keep, t_mlp, total;
};

// the q/k/v adapters' dropout masks travel from the forward to the backward as keep bits (2 bytes per float4 of the
// LayerNorm output, clipfs_lora_keep_bits_ok) instead of being regenerated from Philox in the dA and dx products
static inline bool keep_bits_slot(const clipfs_tower* t) {  // the slot exists (layout: independent of the step's seed)
  return t->lora_r > 0 && t->lora_dropout > 0.f && clipfs_lora_keep_bits_ok(t->width, t->width, t->lora_r, 3);
}
static inline bool keep_bits_saved(const clipfs_tower* t) { return keep_bits_slot(t) && t->dropout_seed != 0; }

// One saved record of `rows` per-row entries: rows = batch * seq for the dense forward, the plan's R live rows for
// clipfs_tower_fwd_packed (no larger than the dense record for R <= M).  The lse slot keeps its
// [sequence * heads + head][seq] layout whatever the row count.
static SavedLayout saved_layout_rows(const clipfs_tower* t, size_t M, size_t batch) {
  const size_t d = t->width, r = t->lora_r > 0 ? t->lora_r : 0;
  SavedLayout L;
  size_t o = 0;
  L.x_in = o;  o += al4(M * d);
  L.stat1 = o; o += al4(2 * M);
  L.h1 = o;    o += al4(M * d);
  L.t_qkv = o; o += al4(M * 3 * r);
  L.qkv = o;   o += al4(qkv_f16(t) ? (M * 3 * d + 1) / 2 : M * 3 * d);  // fp16 mode: q | k | v saved as f16
  L.att = o;   o += al4(M * d);
  // log-sum-exp rows (batch * seq * heads floats in either mode): every backward with statistics reads them
  L.lse = o;   o += al4(t->weight_format == 2 ? batch * t->seq * (size_t)t->heads
                                              : clipfs_attention_lse_floats((int)batch, t->seq, t->heads));
  L.t_o = o;   o += al4(M * r);
  L.x_mid = o; o += al4(M * d);
  L.stat2 = o; o += al4(2 * M);
  L.u = o;     o += al4(t->weight_format == 2 ? M * 2 * d : M * 4 * d);  // fp16 mode: pre-activation saved as f16
  L.keep = o;  o += keep_bits_slot(t) ? al4((M * (d / 4) + 1) / 2) : 0;    // uint16 per float4 of h1
  // towers with an MLP adapter only: t_fc | t_pr, the two down-projections [M, r] each
  L.t_mlp = o; o += tower_has_mlp_lora(t) ? 2 * al4(M * r) : 0;
  L.total = o;
  return L;
}

// bias gradient slots (clipfs_block.g_*): NULL everywhere = bias='none', and then the backward launches exactly what it
// launched before they existed
static inline bool block_has_bias_slots(const clipfs_block& b) {
  return b.g_ln1_b || b.g_ln2_b || b.g_b_q || b.g_b_k || b.g_b_v || b.g_b_o || b.g_b_fc || b.g_b_pr;
}
static bool tower_has_bias_slots(const clipfs_tower* t) {
  if (!t->blocks || t->block_size != sizeof(clipfs_block)) return false;
  for (int l = 0; l < t->layers; ++l)
    if (block_has_bias_slots(t->blocks[l])) return true;
  return false;
}

// (N, K) of a block's GEMMs in units of the width: QKV, out-projection, c_fc, c_proj, then the backward's dgrads into
// LayerNorm 1's output, the pre-activation and the attention output (c_fc's dgrad has c_proj's shape)
constexpr int kFwdGemms = 4, kGemms = 7;
constexpr int kGemmShape[kGemms][2] = {{3, 1}, {1, 1}, {4, 1}, {1, 4}, {1, 3}, {4, 1}, {1, 1}};

struct ScratchLayout {
  size_t h, big, b3, b1, dt, work, gemm_ws, gemm_ws_floats, a16, c16, bwork, total;
  size_t counter_ints;  // split-K arrival counters the tower's largest GEMM needs (a separate, caller-zeroed buffer)
};

static ScratchLayout scratch_layout(const clipfs_tower* t, size_t M) {
  const size_t d = t->width, r = t->lora_r > 0 ? t->lora_r : 0;
  ScratchLayout S;
  size_t o = 0;
  S.h = o;    o += al4(M * d);
  S.big = o;  o += al4(M * 4 * d);
  S.b3 = o;   o += al4(M * 3 * d);
  S.b1 = o;   o += al4(M * d);
  S.dt = o;   o += al4(M * 4 * r);
  size_t lw = r ? al4(clipfs_lora_bwd_work_floats((int)M, (int)d, (int)r, 3)) : 0;
  if (r && tower_has_mlp_lora(t)) {  // the d -> 4d and 4d -> d adapters' slice plans
    const size_t w_fc = al4(clipfs_lora_bwd_work_floats2((int)M, (int)d, 4 * (int)d, (int)r, 1));
    const size_t w_pr = al4(clipfs_lora_bwd_work_floats2((int)M, 4 * (int)d, (int)d, (int)r, 1));
    lw = w_fc > lw ? w_fc : lw;
    lw = w_pr > lw ? w_pr : lw;
  }
  S.work = o; o += lw;
  // split-K scratch for the largest of the tower's GEMM shapes (0 unless the row count is small)
  size_t ws = 0, cnt = 0;
  // ... at the tower's row count and at one row per sequence (the compact last block: clipfs_tower_fwd_rows /
  // clipfs_tower_bwd_sparse run their products on `batch` rows)
  const size_t row_counts[2] = {M, M / (size_t)t->seq};
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < kGemms; ++i) {
      if (!row_counts[k]) continue;
      const int N = kGemmShape[i][0] * (int)d, K = kGemmShape[i][1] * (int)d;
      const size_t w = clipfs_gemm_workspace_floats((int)row_counts[k], N, K);
      const size_t c = clipfs_gemm_counter_ints((int)row_counts[k], N, K);
      ws = w > ws ? w : ws;
      cnt = c > cnt ? c : cnt;
    }
  S.counter_ints = cnt;
  S.gemm_ws = o; S.gemm_ws_floats = ws; o += al4(ws);
  // fp16 storage mode (weight_format 2): f16 images of the GEMM operands, M x 4d halves each
  S.a16 = o; o += t->weight_format == 2 ? al4(M * 2 * d) : 0;
  S.c16 = o; o += t->weight_format == 2 ? al4(M * 2 * d) : 0;
  // partial slab of the bias-gradient column sums (clipfs_bias_grad), only when some block has a bias slot
  size_t bw = 0;
  if (tower_has_bias_slots(t)) {
    const int widths[3] = {(int)d, 3 * (int)d, 4 * (int)d};
    for (int k = 0; k < 2; ++k)
      for (int i = 0; i < 3; ++i) {
        if (!row_counts[k]) continue;
        const size_t w = clipfs_bias_grad_work_floats((int)row_counts[k], widths[i]);
        bw = w > bw ? w : bw;
      }
  }
  S.bwork = o; o += al4(bw);
  S.total = o;
  return S;
}

static int check_tower(const clipfs_tower* t, int batch) {
  CLIPFS_REQUIRE(t && t->blocks, "tower: null descriptor");
  CLIPFS_REQUIRE(t->struct_size == sizeof(clipfs_tower) && t->block_size == sizeof(clipfs_block),
                 "tower: descriptor built against another clipfs.h (struct_size %zu / block_size %zu, library has %zu / %zu)",
                 t->struct_size, t->block_size, sizeof(clipfs_tower), sizeof(clipfs_block));
  CLIPFS_REQUIRE(batch > 0 && t->layers > 0 && t->seq > 0 && t->heads > 0 && t->width == t->heads * 64,
                 "tower: width %d must be heads %d * 64", t->width, t->heads);
  CLIPFS_REQUIRE(t->lora_r >= 0 && t->lora_r <= 64, "tower: lora rank %d unsupported (0..64) at width %d", t->lora_r,
                 t->width);
  // ranks above 16: the adapter kernels' plan says whether a family takes them at this width
  struct clipfs_lora_plan lp;
  CLIPFS_REQUIRE(t->lora_r <= 16 || clipfs_lora_plan(CLIPFS_LORA_OP_BWD, 1, t->width, t->width, t->lora_r, 3, 0, &lp) == CLIPFS_OK,
                 "tower: lora rank %d at width %d unsupported (ranks above 16 need a width that is a multiple of 128)",
                 t->lora_r, t->width);
  CLIPFS_REQUIRE(t->grad_lo >= 0 && t->grad_lo < t->layers, "tower: grad_lo %d outside [0, layers %d)", t->grad_lo,
                 t->layers);
  // blocks below the floor get no backward: a gradient slot there would silently stay untouched
  for (int l = 0; l < t->grad_lo; ++l) {
    const clipfs_block& b = t->blocks[l];
    CLIPFS_REQUIRE(!b.g_lora_a_qkv && !b.g_lora_b_qkv && !b.g_lora_a_o && !b.g_lora_b_o && !b.g_lora_a_fc && !b.g_lora_b_fc &&
                       !b.g_lora_a_pr && !b.g_lora_b_pr && !block_has_bias_slots(b) && !b.g_prompt,
                   "tower: block %d below grad_lo %d has gradient slots", l, t->grad_lo);
  }
  for (int l = 0; l < t->layers; ++l) {  // deep prompts (clipfs_block.prompt)
    const clipfs_block& b = t->blocks[l];
    CLIPFS_REQUIRE(b.prompt || !b.g_prompt, "tower: block %d has a prompt gradient slot but no prompt", l);
    CLIPFS_REQUIRE(!b.prompt || (b.prompt_first >= 0 && b.prompt_rows > 0),
                   "tower: block %d prompt rows first %d count %d", l, b.prompt_first, b.prompt_rows);
  }
  for (int l = 0; l < t->layers; ++l) {  // MLP adapters (clipfs_block.lora_a_fc / lora_a_pr)
    const clipfs_block& b = t->blocks[l];
    const Adapters ad = adapters(b);
    if (!ad.mlp()) continue;
    CLIPFS_REQUIRE(t->lora_r > 0, "tower: block %d has an MLP adapter but lora_r is 0", l);
    CLIPFS_REQUIRE(!ad.fc || b.lora_b_fc, "tower: block %d c_fc adapter lacks its B matrix", l);
    CLIPFS_REQUIRE(!ad.pr || b.lora_b_pr, "tower: block %d c_proj adapter lacks its B matrix", l);
    // h2, g and du exist only as f16 images in the fp16 storage mode: nothing the adapter products could read
    CLIPFS_REQUIRE(t->weight_format != 2, "tower: block %d has a %s adapter: MLP adapters are not supported in the fp16 storage mode",
                   l, ad.fc ? "c_fc" : "c_proj");
  }
  if (t->weight_format == 2)  // fp16 storage mode chains f16 results between GEMMs: every block needs all its f16 weights
    for (int l = 0; l < t->layers; ++l) {
      const clipfs_block& b = t->blocks[l];
      CLIPFS_REQUIRE(b.w_qkv_p && b.w_o_p && b.w_fc_p && b.w_pr_p, "tower: block %d lacks f16 weight copies", l);
      // dqkv and the MLP gradient exist only as f16 images there: nothing to take the bias column sums of
      CLIPFS_REQUIRE(!block_has_bias_slots(b), "tower: bias gradients are not supported in the fp16 storage mode (block %d)",
                     l);
    }
  return CLIPFS_OK;
}

// Every block the backward walks needs its transposed weights, and in fp16 storage mode their f16 planes (dqkv and the
// MLP gradient exist only as f16 images there: the fp32 dgrad would read a tensor nobody wrote).  Checked before the
// first launch of every backward entry point.
static int check_bwd_weights(const clipfs_tower* t) {
  for (int l = t->grad_lo; l < t->layers; ++l) {
    const clipfs_block& b = t->blocks[l];
    CLIPFS_REQUIRE(b.w_pr_t && b.w_fc_t && b.w_o_t && b.w_qkv_t, "tower_bwd: block %d lacks transposed weights", l);
    CLIPFS_REQUIRE(t->weight_format != 2 || (b.w_pr_t_p && b.w_fc_t_p && b.w_o_t_p && b.w_qkv_t_p),
                   "tower_bwd: block %d lacks f16 copies of the transposed weights", l);
  }
  return CLIPFS_OK;
}

// Per-call state of a tower pass (no hidden / thread-local state: everything a GEMM of the pass needs travels here)
struct TowerCtx {
  float* ws = nullptr;          // split-K scratch (inside the call's scratch buffer)
  size_t ws_floats = 0;
  int* counters = nullptr;      // split-K arrival counters (caller-zeroed; every launch leaves them zero)
  size_t counters_ints = 0;
  int b_format = 0;             // format of the blocks' 16-bit weight copies
  void* a16 = nullptr;          // fp16 mode: f16 image of the A operand (converted per GEMM)
  void* c16 = nullptr;          // fp16 mode: f16 output handed from one GEMM to the next
};

static TowerCtx make_ctx(const clipfs_tower* t, float* scratch, const ScratchLayout& SC) {
  TowerCtx c;
  c.ws = scratch + SC.gemm_ws;
  c.ws_floats = SC.gemm_ws_floats;
  c.counters = t->gemm_counters;
  c.counters_ints = t->gemm_counters_ints;
  c.b_format = t->weight_format;
  c.a16 = t->weight_format == 2 ? scratch + SC.a16 : nullptr;
  c.c16 = t->weight_format == 2 ? scratch + SC.c16 : nullptr;
  return c;
}

enum GemmChain { CHAIN_NONE = 0, CHAIN_OUT16 = 1, CHAIN_IN16 = 2 };

// C[M, N] = A[M, K] B[N, K]^T (+ epilogue).  The first seven fields are mandatory, everything else defaults to "none".
struct Gemm {
  int M, N, K;
  const float* A;
  const float* B;
  const void* planes;               // B's 16-bit copies (NULL: the fp32 master weights)
  float* C;
  const float* bias = nullptr;
  const float* residual = nullptr;  // [M, N], added in the epilogue
  int act = 0;                      // 1 = QuickGELU (pre-activation to aux_out), 2 = times gelu'(aux_in)
  float* aux_out = nullptr;
  const float* aux_in = nullptr;
  struct {                          // adapter up-projection folded into the epilogue: t [M, nseg * r] (NULL = none)
    const float* t = nullptr;
    const float* b = nullptr;
    int r = 0, nseg = 0, segw = 0;
    float scale = 0.f;
  } lora;
  // CHAIN_OUT16 = the result is only the next GEMM's A operand: in fp16 mode write it as f16 alone;
  // CHAIN_IN16  = A is the previous GEMM's CHAIN_OUT16 result
  int chain = CHAIN_NONE;
  const void* a16_ready = nullptr;  // f16 image of A written by the producing kernel (LayerNorm / attention); NULL = convert here
  void* c16_only = nullptr;         // fp16 mode: keep the result as f16 alone, here (qkv, dO)
};

static int gemm(const TowerCtx& cx, const Gemm& g, hipStream_t st) {
  clipfs_gemm_args a = {};
  a.struct_size = sizeof(a);
  a.B_planes = g.planes;
  a.b_format = cx.b_format;
  a.workspace = cx.ws;
  a.workspace_floats = cx.ws_floats;
  a.counters = cx.counters;
  a.counters_ints = cx.counters_ints;
  a.A = g.A; a.B = g.B; a.C = g.C; a.M = g.M; a.N = g.N; a.K = g.K;
  a.lda = g.K; a.ldb = g.K; a.ldc = g.N; a.alpha = 1.f;
  a.bias = g.bias; a.residual = g.residual; a.ldres = g.N;
  a.act = g.act; a.aux_out = g.aux_out; a.aux_in = g.aux_in;
  a.lora_t = g.lora.t; a.lora_b = g.lora.b; a.lora_r = g.lora.r; a.lora_nseg = g.lora.nseg;
  a.lora_seg_width = g.lora.segw; a.lora_scale = g.lora.scale;
  if (cx.b_format == 2 && g.planes && cx.a16 && (g.K % 32) == 0 &&
      (!g.lora.t || (g.lora.segw % 128 == 0 && g.lora.r <= 64))) {
    if (g.chain & CHAIN_IN16) {
      a.A_f16 = cx.c16;
    } else if (g.a16_ready) {
      a.A_f16 = g.a16_ready;  // the producing kernel already wrote the f16 image
    } else {
      CLIPFS_CHECK(clipfs_convert_f16(g.A, cx.a16, (size_t)g.M * g.K, st));
      a.A_f16 = cx.a16;
    }
    if (g.chain & CHAIN_OUT16) {
      a.C_f16 = cx.c16;
      a.C = nullptr;
    }
    a.aux_f16 = 1;  // fp16 storage of the saved pre-activation (only the f16 x f16 GEMMs read or write it)
    if (g.c16_only) {
      a.C_f16 = g.c16_only;
      a.C = nullptr;
    }
  } else {
    CLIPFS_REQUIRE(!g.c16_only, "tower: the f16 x f16 GEMM is required for an f16-only result");
  }
  return clipfs_gemm_nt(&a, st);
}

// Which rows a walk runs on.  Three views exist: every row (dense); the live rows of a plan over the dense forward's
// saved records (clipfs_tower_bwd_packed); the live rows over clipfs_tower_fwd_packed's own records.
//
// The plan (int32, device) of a causal tower: sequence c carries gradient on its rows c*seq + 0 .. eot_c only (the head
// reads its EOT row and a row never attends to a later one), and forward the same rows are all the head depends on: the
// R = sum (eot_c + 1) live rows are packed caption after caption.  off[0 .. batch] is the exclusive prefix sum of
// eot_c + 1 (off[batch] = R), eotp[0 .. batch) = off[c + 1] - 1 the packed row of each EOT, map[0 .. R) = c * seq + p the
// full-layout row of packed row i.
struct RowView {
  int n = 0;                      // rows of the walk: batch * seq, or R
  int srows = 0;                  // rows of a saved record (offset of the rstd half of a statistics slot)
  const int32_t* map = nullptr;   // NULL = dense rows
  const int32_t* off = nullptr;
  const int32_t* eotp = nullptr;
  bool gather = false;            // the saved records are dense: their live rows are gathered through map into scratch
  TowerCtx cx;                    // context of the n-row GEMMs
  bool packed() const { return map != nullptr; }
  bool saved_packed() const { return map && !gather; }
};

// Which attention a block runs: decided here alone, read by fwd_block, bwd_attn_half and pack_ok.
enum class AttnRoute {
  Fp32Dense,     // clipfs_attention_fwd / _bwd
  Fp32Packed,    // live rows over dense records: clipfs_attention_bwd_packed
  Fp32PackedIo,  // live rows over packed records: clipfs_attention_fwd_packed / _bwd_packed_io
  F16Dense,      // fp16 storage mode: clipfs_attention_f16_fwd / _bwd
  F16Packed,     // ... live rows over dense records: clipfs_attention_f16_bwd_packed
  Fp32Fallback,  // fp16 storage mode past the f16 kernels' bound: the dense fp32 pair (never packed: pack_ok)
};
static AttnRoute attn_route(const clipfs_tower* t, bool packed, bool saved_packed) {
  if (t->weight_format == 2) {  // (the live-row forward is exact fp32 only, pack_fwd_ok: no packed records here)
    if (!f16_attention(t)) return AttnRoute::Fp32Fallback;
    return packed ? AttnRoute::F16Packed : AttnRoute::F16Dense;
  }
  if (saved_packed) return AttnRoute::Fp32PackedIo;
  return packed ? AttnRoute::Fp32Packed : AttnRoute::Fp32Dense;
}
static AttnRoute attn_route(const clipfs_tower* t, const RowView& v) { return attn_route(t, v.packed(), v.saved_packed()); }

// One call's state, built by begin_pass
struct Pass {
  const clipfs_tower* t;
  int batch, M;
  float* scratch;
  hipStream_t st;
  ScratchLayout SC;
  TowerCtx cx;          // the dense rows' and the compact `batch`-row products' GEMM context
  void* dqkv16;         // fp16 mode: [M, 3d] halves behind the [M, d] image at cx.a16
  const int32_t* plan;  // the live-row entry points' plan and its R
  int R;
  RowView v;
  SavedLayout SL;       // of the view's saved records
};

// The checks the entry points share; nothing is enqueued here.  buffers: the entry point's pointer arguments are all
// there; stop_at_input: NULL for a forward; plan / R: of the live-row entry points (NULL / 0 elsewhere).
static int begin_pass(Pass* p, const char* who, const clipfs_tower* t, int batch, bool buffers, const int* stop_at_input,
                      const int32_t* plan, int R, float* scratch, void* stream) {
  CLIPFS_CHECK(check_tower(t, batch));
  CLIPFS_REQUIRE(!stop_at_input || t->grad_lo == 0 || *stop_at_input,
                 "%s: grad_lo %d > 0 needs stop_at_input (the input gradient runs through every block)", who, t->grad_lo);
  CLIPFS_REQUIRE(buffers, "%s: null buffer", who);
  const int M = batch * t->seq;
  CLIPFS_REQUIRE(!plan || (R >= batch && R <= M), "%s: R %d outside [batch %d, batch*seq %d]", who, R, batch, M);
  *p = Pass{t, batch, M, scratch, (hipStream_t)stream, scratch_layout(t, (size_t)M)};
  CLIPFS_REQUIRE(!t->gemm_counters || t->gemm_counters_ints >= p->SC.counter_ints,
                 "tower: gemm_counters holds %zu ints, %zu needed", t->gemm_counters_ints, p->SC.counter_ints);
  p->cx = make_ctx(t, scratch, p->SC);
  p->dqkv16 = p->cx.a16 ? (void*)((char*)p->cx.a16 + (size_t)M * t->width * 2) : nullptr;
  p->plan = plan;
  p->R = R;
  p->v.n = p->v.srows = M;  // the dense view, unless packed_rows follows
  p->v.cx = p->cx;
  p->SL = saved_layout_rows(t, (size_t)M, (size_t)batch);
  return CLIPFS_OK;
}

// saved_packed: the saved records are the live-row forward's.  unsplit: the R-row GEMMs run without split-K -- the K
// order of one output element depends on the split factor only, never on the tile height, so an unsplit R-row launch
// reproduces the unsplit dense launch bitwise (pack_fwd_ok)
static void packed_rows(Pass* p, bool saved_packed, bool unsplit) {
  const int32_t* plan = p->plan;
  p->v.n = p->R;
  p->v.srows = saved_packed ? p->R : p->M;
  p->v.off = plan;
  p->v.eotp = plan + p->batch + 1;
  p->v.map = plan + 2 * (size_t)p->batch + 1;
  p->v.gather = !saved_packed;
  p->v.cx = p->cx;
  if (unsplit) {
    p->v.cx.ws = nullptr;
    p->v.cx.counters = nullptr;
    p->v.cx.ws_floats = p->v.cx.counters_ints = 0;
  }
  p->SL = saved_layout_rows(p->t, (size_t)p->v.srows, (size_t)p->batch);
}

// the packed walks keep their residual stream (forward: x, backward: dx) in the second half of the b1 slot, the
// attention output / its gradient in the first half (R <= M / 2, pack_ok)
static float* packed_x(const Pass& p) { return p.scratch + p.SC.b1 + al4((size_t)p.v.n * p.t->width); }

// A per-row saved tensor ([srows, w] floats) as the view's walk reads it: in place, or -- live rows over dense records --
// gathered into `slot`
static int saved_rows(const Pass& p, const float* src, int w, float* slot, const float** out) {
  *out = src;
  if (!p.v.gather) return CLIPFS_OK;
  *out = slot;
  return clipfs_gather_rows_map(src, (size_t)w, p.v.map, slot, p.v.n, w, p.st);
}

// where the backward gathers them (the MLP scratch, dead by then): h1 / t_qkv / keep bits, and att / t_o for an
// o-projection adapter
struct GatherSlots {
  float *h1, *t_qkv, *keep, *att, *t_o;
};
static GatherSlots gather_slots(const Pass& p) {
  const size_t R = (size_t)p.v.n, d = p.t->width, r = p.t->lora_r;
  GatherSlots g;
  g.h1 = p.scratch + p.SC.big;
  g.t_qkv = g.h1 + al4(R * d);
  g.keep = g.t_qkv + al4(R * 3 * r);
  g.att = g.keep + al4(R * d / 8);
  g.t_o = g.att + al4(R * d);
  return g;
}

// The compact (one row per sequence) part of the last block picks its `batch` rows of a [rows, w] tensor, and puts them
// back, either at rows[c] within sequence c of the full layout or -- packed records -- at the plan's EOT rows.
// f16: the tensor holds halves (the saved pre-activation in fp16 storage mode).
static int pick_rows(const Pass& p, const int32_t* rows, const float* src, int w, float* dst, bool f16 = false) {
  if (p.v.saved_packed()) return clipfs_gather_rows_map(src, (size_t)w, p.v.eotp, dst, p.batch, w, p.st);
  if (f16) return clipfs_gather_seq_rows_f16(src, (size_t)w, rows, dst, p.batch, p.t->seq, w, p.st);
  return clipfs_gather_seq_rows(src, (size_t)w, rows, dst, p.batch, p.t->seq, w, p.st);
}
static int put_rows(const Pass& p, const int32_t* rows, const float* src, int w, float* dst, bool f16 = false) {
  if (p.v.saved_packed()) return clipfs_put_rows_map(src, p.v.eotp, dst, (size_t)w, p.batch, w, p.st);
  if (f16) return clipfs_put_seq_rows_f16(src, rows, dst, (size_t)w, p.batch, p.t->seq, w, p.st);
  return clipfs_put_seq_rows(src, rows, dst, (size_t)w, p.batch, p.t->seq, w, p.st);
}

// deep prompt of block b (clipfs_block.prompt): written over its rows of the block input x (through the view's offsets
// on packed rows); its gradient taken from the input gradient dx (and those rows of dx / its f16 image zeroed: the
// replaced rows do not depend on the block below)
static int put_prompt(const Pass& p, const clipfs_block& b, float* x) {
  if (!b.prompt) return CLIPFS_OK;
  return clipfs_prompt_put(b.prompt, x, p.v.off, p.batch, p.t->seq, b.prompt_first, b.prompt_rows, p.t->width, p.st);
}
static int harvest_prompt(const Pass& p, const clipfs_block& b, float* dx, void* dx16) {
  if (!b.prompt) return CLIPFS_OK;
  return clipfs_prompt_harvest(dx, dx16, p.v.off, p.batch, p.t->seq, b.prompt_first, b.prompt_rows, p.t->width, b.g_prompt,
                               p.st);
}

// accumulate the column sums of a dense [rows, cols] tensor into up to three bias slots (nothing when all are NULL)
static int bias_sum(const Pass& p, const float* x, int rows, int cols, int segw, float* o0, float* o1 = nullptr,
                    float* o2 = nullptr) {
  if (!o0 && !o1 && !o2) return CLIPFS_OK;
  return clipfs_bias_grad(x, (size_t)cols, rows, cols, segw, o0, o1, o2, p.scratch + p.SC.bwork, p.st);
}

// LayerNorm over the view's rows.  stat: the saved mean | rstd slot (forward: NULL = not kept); y16: fp16 mode, the f16
// image of the result for the next GEMM.
static int ln_fwd(const Pass& p, const float* x, const float* g, const float* be, float* y, void* y16, float* stat) {
  const int d = p.t->width;
  float* rstd = stat ? stat + p.v.srows : nullptr;
  if (y16) return clipfs_layernorm_fwd_f16(x, d, g, be, y, y16, stat, rstd, p.v.n, d, 1e-5f, p.st);
  return clipfs_layernorm_fwd(x, d, g, be, y, stat, rstd, p.v.n, d, 1e-5f, p.st);
}
// out = res + LN'(dy); x and its statistics are read in place, through the row map where the records are dense and the
// rows packed
static int ln_bwd(const Pass& p, const float* dy, const float* x, const float* g, const float* stat, const float* res,
                  float* out, void* out16) {
  const int d = p.t->width;
  const float* rstd = stat + p.v.srows;
  if (p.v.gather && out16)
    return clipfs_layernorm_bwd_rows_f16(dy, x, d, g, stat, rstd, p.v.map, res, out, out16, d, p.v.n, d, p.st);
  if (p.v.gather) return clipfs_layernorm_bwd_rows(dy, x, d, g, stat, rstd, p.v.map, res, out, d, p.v.n, d, p.st);
  if (out16) return clipfs_layernorm_bwd_f16(dy, x, d, g, stat, rstd, res, out, out16, d, p.v.n, d, p.st);
  return clipfs_layernorm_bwd(dy, x, d, g, stat, rstd, res, out, d, p.v.n, d, p.st);
}

}  // namespace clipfs

using namespace clipfs;

extern "C" size_t clipfs_tower_saved_floats(const clipfs_tower* t, int batch) {
  if (!t || batch <= 0 || t->struct_size != sizeof(clipfs_tower)) return 0;
  if (t->grad_lo < 0 || t->grad_lo >= t->layers) return 0;
  // blocks grad_lo ... top
  return saved_layout_rows(t, (size_t)batch * t->seq, (size_t)batch).total * (size_t)(t->layers - t->grad_lo);
}

extern "C" size_t clipfs_tower_scratch_floats(const clipfs_tower* t, int batch) {
  if (!t || batch <= 0 || t->struct_size != sizeof(clipfs_tower)) return 0;
  return scratch_layout(t, (size_t)batch * t->seq).total;
}

extern "C" size_t clipfs_tower_counter_ints(const clipfs_tower* t, int batch) {
  if (!t || batch <= 0 || t->struct_size != sizeof(clipfs_tower)) return 0;
  return scratch_layout(t, (size_t)batch * t->seq).counter_ints;
}

// Last block "one row per sequence" mode (clipfs_tower_fwd_rows / clipfs_tower_bwd_sparse): both directions must agree,
// the compact forward leaves the skipped rows of x_mid / u / stat2 unwritten.
static bool last_block_rows_ok(const clipfs_tower* t) {
  static const bool force_dense = getenv("CLIPFS_DENSE_BWD") && atoi(getenv("CLIPFS_DENSE_BWD")) != 0;  // A/B aid
  const Adapters ad = adapters(t->blocks[t->layers - 1]);
  return !(force_dense || ad.o || ad.mlp() || t->seq < 8);
}

// ---- forward -------------------------------------------------------------------------------------------------------

// The rest of the LAST block on one row per sequence: the head reads nothing else (jclip/model.py:121-124, :213-214) and
// every remaining operation is row-wise.  att / x_in: the block's attention output and input on the view's rows.  The
// compact buffers live in the MLP scratch (batch (13 d + 2) floats <= M 4 d for seq >= 4); what the backward's compact
// head picks again (x_mid, u, LayerNorm-2 statistics) is put back at those rows of the saved record sv (NULL: nothing
// is kept), the block output at rows[c] of x.
static int fwd_tail(const Pass& p, const clipfs_block& b, float* sv, const float* att, const float* x_in,
                    const int32_t* rows, float* x) {
  const clipfs_tower* t = p.t;
  const int d = t->width, Ms = p.batch;
  const SavedLayout& SL = p.SL;
  const size_t Md = (size_t)Ms * d;
  float* at = p.scratch + p.SC.big;
  auto take = [&at](size_t floats) { float* q = at; at += floats; return q; };
  float *att_s = take(Md), *xin_s = take(Md), *xmid_s = take(Md), *h2_s = take(Md), *xout_s = take(Md);
  float *g_s = take(4 * Md), *u_s = take(4 * Md), *mean_s = take(al4((size_t)Ms)), *rstd_s = take((size_t)Ms);
  CLIPFS_CHECK(pick_rows(p, rows, att, d, att_s));
  CLIPFS_CHECK(pick_rows(p, rows, x_in, d, xin_s));
  // fp16 storage mode: these `batch`-row products use the fp32 master weights (plane argument NULL) -- the f16 kernels
  // are built for tens of thousands of rows -- and the pre-GELU rows go back into the f16 tensor the dense path keeps
  const bool f16m = t->weight_format == 2;
  CLIPFS_CHECK(gemm(p.cx, {.M = Ms, .N = d, .K = d, .A = att_s, .B = b.w_o, .planes = f16m ? nullptr : b.w_o_p, .C = xmid_s,
                           .bias = b.b_o, .residual = xin_s}, p.st));
  CLIPFS_CHECK(clipfs_layernorm_fwd(xmid_s, d, b.ln2_g, b.ln2_b, h2_s, sv ? mean_s : nullptr, sv ? rstd_s : nullptr, Ms, d,
                                    1e-5f, p.st));
  CLIPFS_CHECK(gemm(p.cx, {.M = Ms, .N = 4 * d, .K = d, .A = h2_s, .B = b.w_fc, .planes = f16m ? nullptr : b.w_fc_p, .C = g_s,
                           .bias = b.b_fc, .act = 1, .aux_out = sv ? u_s : nullptr}, p.st));
  CLIPFS_CHECK(gemm(p.cx, {.M = Ms, .N = d, .K = 4 * d, .A = g_s, .B = b.w_pr, .planes = f16m ? nullptr : b.w_pr_p, .C = xout_s,
                           .bias = b.b_pr, .residual = xmid_s}, p.st));
  CLIPFS_CHECK(clipfs_put_seq_rows(xout_s, rows, x, (size_t)d, Ms, t->seq, d, p.st));
  if (!sv) return CLIPFS_OK;
  CLIPFS_CHECK(put_rows(p, rows, xmid_s, d, sv + SL.x_mid));
  CLIPFS_CHECK(put_rows(p, rows, u_s, 4 * d, sv + SL.u, f16m));
  CLIPFS_CHECK(put_rows(p, rows, mean_s, 1, sv + SL.stat2));
  return put_rows(p, rows, rstd_s, 1, sv + SL.stat2 + p.v.srows);
}

// Block l on the view's rows.  A block from the gradient floor up keeps its activations in saved record l - grad_lo (when
// saved != NULL) and hands its output to the next record's x_in; the others work in the residual stream xr -- x itself,
// or the packed rows -- in place.  rows != NULL: the compact tail follows the last block's attention.
static int fwd_block(const Pass& p, int l, float* x, const int32_t* rows, float* saved) {
  const clipfs_tower* t = p.t;
  const clipfs_block& b = t->blocks[l];
  const RowView& v = p.v;
  const SavedLayout& SL = p.SL;
  const ScratchLayout& SC = p.SC;
  const int n = v.n, d = t->width, r = t->lora_r;
  hipStream_t st = p.st;
  const int lo = t->grad_lo;
  const bool train = saved != nullptr, keep_l = train && l >= lo;
  float* sv = keep_l ? saved + (size_t)(l - lo) * SL.total : nullptr;
  float* xr = v.packed() ? packed_x(p) : x;
  float* x_next = keep_l && l + 1 < t->layers ? saved + (size_t)(l + 1 - lo) * SL.total + SL.x_in : xr;
  float* x_in = sv ? sv + SL.x_in : xr;
  float* h1 = sv ? sv + SL.h1 : p.scratch + SC.h;
  float* qkv = sv ? sv + SL.qkv : p.scratch + SC.b3;
  float* att = sv ? sv + SL.att : p.scratch + SC.b1;
  float* x_mid = sv ? sv + SL.x_mid : xr;
  float* t_qkv = sv ? sv + SL.t_qkv : p.scratch + SC.dt;
  float* t_o = sv ? sv + SL.t_o : p.scratch + SC.dt + al4((size_t)n * 3 * r);
  // attention statistics: kept, or not written at all.  No forward kernel depends on lse (it only guards one store:
  // the plan is the same with and without it, which tests/test_attention_plan.py asserts for every length), so a block
  // below the floor produces bitwise the block output of the saving forward.
  float* lse = sv ? sv + SL.lse : nullptr;
  float* stat1 = sv ? sv + SL.stat1 : nullptr;
  float* stat2 = sv ? sv + SL.stat2 : nullptr;
  const Adapters ad = adapters(b);
  // dropout follows the caller's train MODE (is_training(), lora_train_vlp.py:297-298), carried by a non-zero seed;
  // saving only decides whether activations are kept (a no-grad forward in train mode still drops)
  const uint64_t seed = t->dropout_seed;
  const uint32_t ds = t->dropout_stream0 + 4u * (uint32_t)l;
  CLIPFS_CHECK(put_prompt(p, b, x_in));  // into the saved record, or the residual stream

  // fp16 storage mode: producers write the f16 image of every GEMM operand next to (or instead of) the fp32 tensor
  void* h16 = v.cx.a16;  // [n, d] halves: ln1 / attention / ln2
  void* keep = (sv && ad.qkv_mask && keep_bits_saved(t)) ? (void*)(sv + SL.keep) : nullptr;
  if (ad.qkv_mask && clipfs_layernorm_fwd_lora_ok(d, r, 3)) {
    // small ranks: the adapter's down-projection rides on the LayerNorm pass (the row is in registers there); on packed
    // rows the dropout masks are drawn at the full-layout row, through the map
    float* rstd1 = stat1 ? stat1 + v.srows : nullptr;
    if (v.packed())
      CLIPFS_CHECK(clipfs_layernorm_fwd_lora_map(x_in, d, b.ln1_g, b.ln1_b, h1, h16, stat1, rstd1, n, d, 1e-5f, b.lora_a_qkv,
                                                 t_qkv, r, 3, ad.qkv_mask, t->lora_dropout, seed, ds, t->dropout_row0, v.map,
                                                 keep, st));
    else
      CLIPFS_CHECK(clipfs_layernorm_fwd_lora(x_in, d, b.ln1_g, b.ln1_b, h1, h16, stat1, rstd1, n, d, 1e-5f, b.lora_a_qkv,
                                             t_qkv, r, 3, ad.qkv_mask, t->lora_dropout, seed, ds, t->dropout_row0, keep, st));
  } else {
    CLIPFS_CHECK(ln_fwd(p, x_in, b.ln1_g, b.ln1_b, h1, h16, stat1));
    if (ad.qkv_mask)  // (packed rows: no dropout here, pack_fwd_ok)
      CLIPFS_CHECK(clipfs_lora_down(h1, b.lora_a_qkv, t_qkv, n, d, r, 3, ad.qkv_mask, t->lora_dropout, seed, ds,
                                    t->dropout_row0, keep, st));
  }
  const bool q16 = qkv_f16(t);
  CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = 3 * d, .K = d, .A = h1, .B = b.w_qkv, .planes = b.w_qkv_p, .C = qkv, .bias = b.b_qkv,
                           .lora = {ad.qkv_mask ? t_qkv : nullptr, b.lora_b_qkv, r, 3, d, t->lora_scale},
                           .a16_ready = h16, .c16_only = q16 ? (void*)qkv : nullptr}, st));
  const void* att16 = nullptr;
  switch (attn_route(t, v)) {
    case AttnRoute::Fp32Packed:
    case AttnRoute::Fp32PackedIo:
    case AttnRoute::F16Packed:  // every live-row forward (exact fp32 only: pack_fwd_ok)
      CLIPFS_CHECK(clipfs_attention_fwd_packed(qkv, att, lse, v.off, p.batch, t->seq, t->heads, st));
      break;
    case AttnRoute::F16Dense:
      CLIPFS_CHECK(clipfs_attention_f16_fwd(qkv, q16, att, h16, lse, p.batch, t->seq, t->heads, t->causal, st));
      att16 = h16;
      break;
    default:  // Fp32Dense, Fp32Fallback
      CLIPFS_CHECK(clipfs_attention_fwd(qkv, att, lse, p.batch, t->seq, t->heads, t->causal, st));
  }
  if (rows && l == t->layers - 1) return fwd_tail(p, b, sv, att, x_in, rows, x);
  if (ad.o)  // (packed rows: no dropout here, pack_fwd_ok)
    CLIPFS_CHECK(clipfs_lora_down(att, b.lora_a_o, t_o, n, d, r, 1, 1u, t->lora_dropout, seed, ds + 3, t->dropout_row0, nullptr,
                                  st));
  CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = d, .K = d, .A = att, .B = b.w_o, .planes = b.w_o_p, .C = x_mid, .bias = b.b_o,
                           .residual = x_in, .lora = {ad.o ? t_o : nullptr, b.lora_b_o, r, 1, d, t->lora_scale},
                           .a16_ready = att16}, st));
  float* h2 = p.scratch + SC.h;  // fp16 mode: only the f16 image is consumed (by the c_fc GEMM)
  CLIPFS_CHECK(ln_fwd(p, x_mid, b.ln2_g, b.ln2_b, h16 ? nullptr : h2, h16, stat2));
  float* gbuf = p.scratch + SC.big;
  // MLP adapters (dense rows, never the fp16 storage mode: check_tower, pack_ok): the down-projections read h2 and g in
  // scratch and are kept for the backward; below the floor they live in the dt slot, whose t_qkv / t_o are consumed by now
  float* t_fc = sv ? sv + SL.t_mlp : p.scratch + SC.dt;
  float* t_pr = t_fc + al4((size_t)n * r);
  if (ad.fc)
    CLIPFS_CHECK(clipfs_lora_down(h2, b.lora_a_fc, t_fc, n, d, r, 1, 1u, t->lora_dropout, seed, mlp_stream(t, l), t->dropout_row0,
                                  nullptr, st));
  CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = 4 * d, .K = d, .A = h2, .B = b.w_fc, .planes = b.w_fc_p, .C = gbuf, .bias = b.b_fc,
                           .act = 1, .aux_out = sv ? sv + SL.u : nullptr,
                           .lora = {ad.fc ? t_fc : nullptr, b.lora_b_fc, r, 1, 4 * d, t->lora_scale},
                           .chain = CHAIN_OUT16, .a16_ready = h16}, st));
  if (ad.pr)
    CLIPFS_CHECK(clipfs_lora_down(gbuf, b.lora_a_pr, t_pr, n, 4 * d, r, 1, 1u, t->lora_dropout, seed, mlp_stream(t, l) + 1,
                                  t->dropout_row0, nullptr, st));
  return gemm(v.cx, {.M = n, .N = d, .K = 4 * d, .A = gbuf, .B = b.w_pr, .planes = b.w_pr_p, .C = x_next, .bias = b.b_pr,
                     .residual = x_mid, .lora = {ad.pr ? t_pr : nullptr, b.lora_b_pr, r, 1, d, t->lora_scale},
                     .chain = CHAIN_IN16}, st);
}

// rows == NULL: every block in full.  rows != NULL: the LAST block's output projection, LayerNorm 2 and MLP run on the
// `batch` rows c * seq + rows[c] only (fwd_tail); the packed views always do.
// Packed rows: every value of a live row equals the dense forward's bitwise -- LayerNorm, the adapters and the GEMM
// epilogues are row-wise, the attention masks a dead key exactly as the padding, the dropout masks are drawn at the
// full-layout row (drow0 + map[i]), and each R-row GEMM is launched unsplit.  The block output goes back to x only at
// `rows`.
static int tower_fwd(const Pass& p, float* x, const int32_t* rows, float* saved) {
  const clipfs_tower* t = p.t;
  const SavedLayout& SL = p.SL;
  const bool train = saved != nullptr, packed = p.v.packed();
  const size_t nd = (size_t)p.v.n * t->width;
  const int lo = t->grad_lo;  // gradient floor: blocks below it save nothing (nothing of theirs is back-propagated)
  float* xr = packed ? packed_x(p) : x;
  const bool in_place = packed && train && lo == 0;  // the input is packed straight into the first saved record
  if (packed)
    CLIPFS_CHECK(clipfs_gather_rows_map(x, (size_t)t->width, p.v.map, in_place ? saved + SL.x_in : xr, p.v.n, t->width, p.st));
  for (int l = 0; l < t->layers; ++l) {
    if (train && l == lo && !in_place) {  // the first saved record's input
      hipError_t e = hipMemcpyAsync(saved + SL.x_in, xr, nd * sizeof(float), hipMemcpyDeviceToDevice, p.st);
      CLIPFS_REQUIRE(e == hipSuccess, "tower_fwd: memcpy failed: %s", hipGetErrorString(e));
    }
    CLIPFS_CHECK(fwd_block(p, l, x, rows, saved));
  }
  return CLIPFS_OK;
}

extern "C" int clipfs_tower_fwd(const clipfs_tower* t, float* x, int batch, float* saved, float* scratch, void* stream) {
  Pass p;
  CLIPFS_CHECK(begin_pass(&p, "tower_fwd", t, batch, x && scratch, nullptr, nullptr, 0, scratch, stream));
  return tower_fwd(p, x, nullptr, saved);
}

extern "C" int clipfs_tower_fwd_rows(const clipfs_tower* t, float* x, const int32_t* rows, int batch, float* saved,
                                     float* scratch, void* stream) {
  CLIPFS_REQUIRE(t && rows, "tower_fwd_rows: null argument");
  Pass p;
  CLIPFS_CHECK(begin_pass(&p, "tower_fwd", t, batch, x && scratch, nullptr, nullptr, 0, scratch, stream));
  return tower_fwd(p, x, last_block_rows_ok(t) ? rows : nullptr, saved);
}

extern "C" int clipfs_tower_rows_mode(const clipfs_tower* t) {
  return (t && t->blocks && t->layers > 0 && last_block_rows_ok(t)) ? 1 : 0;
}

// ---- backward ------------------------------------------------------------------------------------------------------

// Adapter backward of one block on the view's rows.  Gradient slots NULL = the adapter is frozen: only its dx
// contribution (when wanted) is computed, and with nothing wanted nothing is launched.
struct LoraBwd {
  const float* dy;
  const void* dy16;  // non-NULL: the output gradient exists as this f16 image alone
  const float* x;    // the adapter's input and its down-projection, as the view reads them (saved_rows)
  const float* tt;
  const float *A, *B;
  float *gA, *gB;
  float* dx;         // accumulated into (NULL: not wanted)
  int nseg;
  unsigned mask;
  uint32_t ds;
  const void* keep;
};
static int lora_bwd_block(const Pass& p, int l, const LoraBwd& a) {
  const clipfs_tower* t = p.t;
  CLIPFS_REQUIRE((a.gA == nullptr) == (a.gB == nullptr), "tower_bwd: block %d has only one of the LoRA gradient slots", l);
  if (!a.gA && !a.dx) return CLIPFS_OK;  // frozen and nothing below needs its input gradient
  const int d = t->width, r = t->lora_r;
  float* dt = p.scratch + p.SC.dt;
  float* work = p.scratch + p.SC.work;
  if (a.dy16)
    return clipfs_lora_bwd_f16dy(a.dy16, a.x, a.tt, a.A, a.B, dt, a.gA, a.gB, a.dx, p.v.n, d, d, r, a.nseg, a.mask,
                                 t->lora_scale, t->lora_dropout, t->dropout_seed, a.ds, t->dropout_row0, a.keep, work, p.st);
  return clipfs_lora_bwd(a.dy, a.x, a.tt, a.A, a.B, dt, a.gA, a.gB, a.dx, p.v.n, d, d, r, a.nseg, a.mask, t->lora_scale,
                         t->lora_dropout, t->dropout_seed, a.ds, t->dropout_row0, a.keep, work, p.st);
}

// fp16 storage mode without an o-projection adapter: the only consumer of the gradient wrt the attention output is the
// f16 attention backward, which rounds dO to f16 for its MFMA operands anyway -- the GEMM writes the f16 image alone (into
// the same scratch slot): a quarter of the epilogue bytes of an fp32 result, half the bytes the attention kernels stage.
// h16: the walk's f16 image of dx (NULL: the walk keeps none)
static inline bool datt_f16(const clipfs_tower* t, const clipfs_block& b, const void* h16) {
  return f16_attention(t) && !adapters(b).o && h16 != nullptr;
}

// a block's input gradient is wanted unless the walk stops at it -- and a trainable prompt needs it even at the floor
static inline bool needs_dx(const clipfs_tower* t, int l, int stop_at_input) {
  return !(l == t->grad_lo && stop_at_input) || t->blocks[l].g_prompt;
}

// Upper half of a block's backward, down to the attention residual: dx (in: the gradient wrt the block output; out: wrt
// x_mid) and the gradient wrt the attention output in the b1 slot.  Slots: big = du (| the gathered u behind it); h = dh.
// Bias gradients are column sums of the tensors below, each taken right after it is written (c_proj: the residual
// gradient entering the block; c_fc: du; ln_2: dh2; out projection: dx after LN2').
static int bwd_mlp_half(const Pass& p, int l, const float* sv, float* dx, void* h16) {
  const clipfs_tower* t = p.t;
  const clipfs_block& b = t->blocks[l];
  const RowView& v = p.v;
  const SavedLayout& SL = p.SL;
  const int n = v.n, d = t->width;
  float* du = p.scratch + p.SC.big;
  float* dh = p.scratch + p.SC.h;
  float* datt = p.scratch + p.SC.b1;
  CLIPFS_CHECK(bias_sum(p, dx, n, d, d, b.g_b_pr));
  // MLP: du = (dx Wpr) * gelu'(u) ; dh2 = du Wfc ; dx += LN2'(dh2)
  // (fp16 storage mode keeps u as halves: 2 d floats per row)
  const float* u;
  CLIPFS_CHECK(saved_rows(p, sv + SL.u, t->weight_format == 2 ? 2 * d : 4 * d, du + 4 * (size_t)n * d, &u));
  const Adapters ad = adapters(b);
  const int r = t->lora_r;
  float* dt = p.scratch + p.SC.dt;
  float* work = p.scratch + p.SC.work;
  if (!ad.pr) {
    CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = 4 * d, .K = d, .A = dx, .B = b.w_pr_t, .planes = b.w_pr_t_p, .C = du, .act = 2,
                             .aux_in = u, .chain = CHAIN_OUT16, .a16_ready = h16}, p.st));
  } else {
    // c_proj adapter: dg = dx Wpr without the activation, the adapter adds (dt_pr A_pr) * dropscale to it and takes dA_pr
    // from QuickGELU(u) read on the fly, then du = dg * gelu'(u) in place.  One route for p = 0 and p > 0.
    CLIPFS_REQUIRE((b.g_lora_a_pr == nullptr) == (b.g_lora_b_pr == nullptr),
                   "tower_bwd: block %d has only one of the c_proj LoRA gradient slots", l);
    CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = 4 * d, .K = d, .A = dx, .B = b.w_pr_t, .planes = b.w_pr_t_p, .C = du}, p.st));
    CLIPFS_CHECK(clipfs_lora_bwd_xact(dx, u, sv + SL.t_mlp + al4((size_t)n * r), b.lora_a_pr, b.lora_b_pr, dt, b.g_lora_a_pr,
                                      b.g_lora_b_pr, du, n, 4 * d, d, r, t->lora_scale, t->lora_dropout, t->dropout_seed,
                                      mlp_stream(t, l) + 1, t->dropout_row0, 1, work, p.st));
    CLIPFS_CHECK(clipfs_gelu_bwd_inplace(du, u, (size_t)n * 4 * d, p.st));
  }
  CLIPFS_CHECK(bias_sum(p, du, n, 4 * d, 4 * d, b.g_b_fc));
  CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = d, .K = 4 * d, .A = du, .B = b.w_fc_t, .planes = b.w_fc_t_p, .C = dh,
                           .chain = CHAIN_IN16}, p.st));
  if (ad.fc) {
    // c_fc adapter: its input h2 = LN2(x_mid) is not saved -- recomputed into the b3 slot (dqkv, not yet written) by the
    // forward's kernel; the adapter's dx term goes into dh2 before LayerNorm 2's backward (and ln_2's bias sum) read it
    CLIPFS_REQUIRE((b.g_lora_a_fc == nullptr) == (b.g_lora_b_fc == nullptr),
                   "tower_bwd: block %d has only one of the c_fc LoRA gradient slots", l);
    float* h2 = p.scratch + p.SC.b3;
    CLIPFS_CHECK(clipfs_layernorm_fwd(sv + SL.x_mid, d, b.ln2_g, b.ln2_b, h2, nullptr, nullptr, n, d, 1e-5f, p.st));
    CLIPFS_CHECK(clipfs_lora_bwd_xact(du, h2, sv + SL.t_mlp, b.lora_a_fc, b.lora_b_fc, dt, b.g_lora_a_fc, b.g_lora_b_fc, dh, n,
                                      d, 4 * d, r, t->lora_scale, t->lora_dropout, t->dropout_seed, mlp_stream(t, l),
                                      t->dropout_row0, 0, work, p.st));
  }
  CLIPFS_CHECK(bias_sum(p, dh, n, d, d, b.g_ln2_b));
  CLIPFS_CHECK(ln_bwd(p, dh, sv + SL.x_mid, b.ln2_g, sv + SL.stat2, dx, dx, h16));
  CLIPFS_CHECK(bias_sum(p, dx, n, d, d, b.g_b_o));
  // attention output projection
  CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = d, .K = d, .A = dx, .B = b.w_o_t, .planes = b.w_o_t_p, .C = datt, .a16_ready = h16,
                           .c16_only = datt_f16(t, b, h16) ? (void*)datt : nullptr}, p.st));
  if (!adapters(b).o) return CLIPFS_OK;
  // (packed rows: no dropout here, pack_dropout_ok -- the adapter backward evaluates no mask)
  const GatherSlots gs = gather_slots(p);
  const float *att, *t_o;
  CLIPFS_CHECK(saved_rows(p, sv + SL.att, d, gs.att, &att));
  CLIPFS_CHECK(saved_rows(p, sv + SL.t_o, t->lora_r, gs.t_o, &t_o));
  return lora_bwd_block(p, l, {.dy = dx, .x = att, .tt = t_o, .A = b.lora_a_o, .B = b.lora_b_o, .gA = b.g_lora_a_o,
                               .gB = b.g_lora_b_o, .dx = datt, .nseg = 1, .mask = 1u,
                               .ds = t->dropout_stream0 + 4u * (uint32_t)l + 3});
}

// Lower half: attention, the QKV projection and LayerNorm 1.  In: the gradient wrt the attention output (b1 slot) and
// wrt the attention residual (dx).  Out: dx = the gradient wrt the block input, when needs_dx.  res_s != NULL (the dense
// rows under the compact head): the residual gradient is zero except on one row per sequence, res_s [batch, d] --
// LayerNorm 1's backward then runs without a residual input, writes every row of dx, and res_s is added at `rows`.
// Slots: b3 = dqkv; h = the D_i work vector of the long-sequence attention kernels, then dh1; big = the gathered
// h1 / t_qkv / keep bits.
static int bwd_attn_half(const Pass& p, int l, const float* sv, float* dx, void* h16, const float* res_s,
                         const int32_t* rows, int stop_at_input) {
  const clipfs_tower* t = p.t;
  const clipfs_block& b = t->blocks[l];
  const RowView& v = p.v;
  const SavedLayout& SL = p.SL;
  const int n = v.n, d = t->width, r = t->lora_r;
  const unsigned qkv_mask = adapters(b).qkv_mask;
  float* dh = p.scratch + p.SC.h;
  float* datt = p.scratch + p.SC.b1;
  float* dqkv = p.scratch + p.SC.b3;
  // fp16 storage mode: the dgrad GEMM and (matrix-core shapes) the adapter backward read the f16 image of dqkv, so the
  // attention backward does not write the fp32 tensor at all (404 MB per ViT-L/14 block at 128 images)
  const bool f16a = f16_attention(t);
  const bool dy16 = f16a && p.dqkv16 && (!qkv_mask || clipfs_lora_bwd_f16dy_ok(d, d, r, 3));
  switch (attn_route(t, v)) {
    case AttnRoute::Fp32PackedIo:  // packed q/k/v and O; packed dO and dqkv either way
      CLIPFS_CHECK(clipfs_attention_bwd_packed_io(sv + SL.qkv, datt, sv + SL.att, sv + SL.lse, dqkv, v.off, p.batch, t->seq,
                                                  t->heads, p.st));
      break;
    case AttnRoute::F16Packed:  // fp16 storage mode: the dense flags, dqkv16 at the packed rows of its slot
      CLIPFS_CHECK(clipfs_attention_f16_bwd_packed(sv + SL.qkv, qkv_f16(t), datt, datt_f16(t, b, h16) ? 1 : 0, sv + SL.att,
                                                   sv + SL.lse, dy16 ? nullptr : dqkv, p.dqkv16, dh, v.off, p.batch, t->seq,
                                                   t->heads, p.st));
      break;
    case AttnRoute::Fp32Packed:
      CLIPFS_CHECK(clipfs_attention_bwd_packed(sv + SL.qkv, datt, sv + SL.att, sv + SL.lse, dqkv, v.off, p.batch, t->seq,
                                               t->heads, p.st));
      break;
    case AttnRoute::F16Dense:
      CLIPFS_CHECK(clipfs_attention_f16_bwd(sv + SL.qkv, qkv_f16(t), datt, datt_f16(t, b, h16) ? 1 : 0, sv + SL.att,
                                            sv + SL.lse, dy16 ? nullptr : dqkv, p.dqkv16, dh, p.batch, t->seq, t->heads,
                                            t->causal, p.st));
      break;
    default:  // Fp32Dense, Fp32Fallback
      CLIPFS_CHECK(clipfs_attention_bwd(sv + SL.qkv, datt, sv + SL.att, sv + SL.lse, dqkv, dh, p.batch, t->seq, t->heads,
                                        t->causal, p.st));
  }
  CLIPFS_CHECK(bias_sum(p, dqkv, n, 3 * d, d, b.g_b_q, b.g_b_k, b.g_b_v));
  const bool need_dx = needs_dx(t, l, stop_at_input);
  // dh1 (the gradient wrt LayerNorm 1's output) is also needed for ln_1's bias gradient, even where dx is not
  const bool need_dh = need_dx || b.g_ln1_b;
  if (need_dh)
    CLIPFS_CHECK(gemm(v.cx, {.M = n, .N = d, .K = 3 * d, .A = dqkv, .B = b.w_qkv_t, .planes = b.w_qkv_t_p, .C = dh,
                             .a16_ready = f16a ? p.dqkv16 : nullptr}, p.st));
  if (qkv_mask) {
    const float *h1 = sv + SL.h1, *t_qkv = sv + SL.t_qkv, *keep = keep_bits_saved(t) ? sv + SL.keep : nullptr;
    if (b.g_lora_a_qkv || need_dh) {  // (frozen and dh not wanted: lora_bwd_block launches nothing)
      const GatherSlots gs = gather_slots(p);
      CLIPFS_CHECK(saved_rows(p, h1, d, gs.h1, &h1));
      CLIPFS_CHECK(saved_rows(p, t_qkv, 3 * r, gs.t_qkv, &t_qkv));
      if (keep) CLIPFS_CHECK(saved_rows(p, keep, d / 8, gs.keep, &keep));  // uint16 per float4 of h1: d / 8 floats per row
    }
    CLIPFS_CHECK(lora_bwd_block(p, l, {.dy = dqkv, .dy16 = dy16 ? p.dqkv16 : nullptr, .x = h1, .tt = t_qkv, .A = b.lora_a_qkv,
                                       .B = b.lora_b_qkv, .gA = b.g_lora_a_qkv, .gB = b.g_lora_b_qkv,
                                       .dx = need_dh ? dh : nullptr, .nseg = 3, .mask = qkv_mask,
                                       .ds = t->dropout_stream0 + 4u * (uint32_t)l, .keep = keep}));
  }
  CLIPFS_CHECK(bias_sum(p, dh, n, d, d, b.g_ln1_b));
  if (!need_dx) return CLIPFS_OK;
  CLIPFS_CHECK(ln_bwd(p, dh, sv + SL.x_in, b.ln1_g, sv + SL.stat1, res_s ? nullptr : dx, dx, h16));
  if (res_s) CLIPFS_CHECK(clipfs_add_seq_rows(res_s, rows, dx, p.batch, t->seq, d, p.st));
  return harvest_prompt(p, b, dx, h16);
}

// blocks l_hi ... grad_lo on the view's rows.  dx [batch*seq, width]: dense rows in/out.  Packed rows: the gradient
// wrt block l_hi's output is in packed_x on entry, and dx receives the gradient wrt the tower input in the full layout
// (unless stop_at_input).
static int bwd_walk(const Pass& p, float* dx, const float* saved, int stop_at_input, int l_hi) {
  const clipfs_tower* t = p.t;
  const int d = t->width;
  float* dxw = p.v.packed() ? packed_x(p) : dx;
  void* h16 = p.v.cx.a16;  // fp16 mode: f16 image of dx; later images come from the LayerNorm backward
  if (h16) CLIPFS_CHECK(clipfs_convert_f16(dxw, h16, (size_t)p.v.n * d, p.st));
  for (int l = l_hi; l >= t->grad_lo; --l) {
    const float* sv = saved + (size_t)(l - t->grad_lo) * p.SL.total;
    CLIPFS_CHECK(bwd_mlp_half(p, l, sv, dxw, h16));
    CLIPFS_CHECK(bwd_attn_half(p, l, sv, dxw, h16, nullptr, nullptr, stop_at_input));
  }
  if (!p.v.packed() || stop_at_input) return CLIPFS_OK;
  // the dead rows are exact zeros
  hipError_t e = hipMemsetAsync(dx, 0, (size_t)p.M * d * sizeof(float), p.st);
  CLIPFS_REQUIRE(e == hipSuccess, "tower_bwd_packed: memset failed: %s", hipGetErrorString(e));
  return clipfs_put_rows_map(dxw, p.v.map, dx, (size_t)d, p.v.n, d, p.st);
}

// The last block's MLP and output projection on the `batch` rows that carry gradient (dxs [batch, d]: the gradient wrt
// the block output at rows[c] of each sequence; every other row's is an exact zero, so the bias gradients are column
// sums over those rows).  Out: the gradient wrt the attention residual and wrt the attention output on those rows.  The
// compact buffers live in the MLP scratch, which this block does not otherwise use: batch (8 d + 4 d + 2) floats
// <= M 4 d for seq >= 3.
static int bwd_head(const Pass& p, const float* sv, const float* dxs, const int32_t* rows, float** dxm_out,
                    float** datt_out) {
  const clipfs_tower* t = p.t;
  const clipfs_block& b = t->blocks[t->layers - 1];
  const SavedLayout& SL = p.SL;
  const int d = t->width, Ms = p.batch;
  const size_t Md = (size_t)Ms * d;
  float* at = p.scratch + p.SC.big;
  auto take = [&at](size_t floats) { float* q = at; at += floats; return q; };
  float *u_s = take(4 * Md), *du_s = take(4 * Md), *xmid_s = take(Md), *dh_s = take(Md), *dxm_s = take(Md);
  float *datt_s = take(Md), *mean_s = take(al4((size_t)Ms)), *rstd_s = take((size_t)Ms);
  CLIPFS_CHECK(bias_sum(p, dxs, Ms, d, d, b.g_b_pr));
  // fp16 storage mode: the `batch`-row products use the fp32 master weights (plane argument NULL); the saved pre-GELU
  // activation is an f16 tensor there
  const bool f16m = t->weight_format == 2;
  CLIPFS_CHECK(pick_rows(p, rows, sv + SL.u, 4 * d, u_s, f16m));
  CLIPFS_CHECK(pick_rows(p, rows, sv + SL.x_mid, d, xmid_s));
  CLIPFS_CHECK(pick_rows(p, rows, sv + SL.stat2, 1, mean_s));
  CLIPFS_CHECK(pick_rows(p, rows, sv + SL.stat2 + p.v.srows, 1, rstd_s));
  CLIPFS_CHECK(gemm(p.cx, {.M = Ms, .N = 4 * d, .K = d, .A = dxs, .B = b.w_pr_t, .planes = f16m ? nullptr : b.w_pr_t_p,
                           .C = du_s, .act = 2, .aux_in = u_s}, p.st));
  CLIPFS_CHECK(bias_sum(p, du_s, Ms, 4 * d, 4 * d, b.g_b_fc));
  CLIPFS_CHECK(gemm(p.cx, {.M = Ms, .N = d, .K = 4 * d, .A = du_s, .B = b.w_fc_t, .planes = f16m ? nullptr : b.w_fc_t_p,
                           .C = dh_s}, p.st));
  CLIPFS_CHECK(bias_sum(p, dh_s, Ms, d, d, b.g_ln2_b));
  CLIPFS_CHECK(clipfs_layernorm_bwd(dh_s, xmid_s, d, b.ln2_g, mean_s, rstd_s, dxs, dxm_s, d, Ms, d, p.st));
  CLIPFS_CHECK(bias_sum(p, dxm_s, Ms, d, d, b.g_b_o));
  *dxm_out = dxm_s;
  *datt_out = datt_s;
  return gemm(p.cx, {.M = Ms, .N = d, .K = d, .A = dxm_s, .B = b.w_o_t, .planes = f16m ? nullptr : b.w_o_t_p, .C = datt_s},
              p.st);
}

// Every backward entry point.  rows == NULL: dx holds the gradient wrt the tower output on every row
// (clipfs_tower_bwd).  rows != NULL: dxs holds it on one row per sequence -- the last block runs bwd_head and then only
// its lower half on the view's rows.
static int tower_bwd(const Pass& p, const float* dxs, const int32_t* rows, float* dx, const float* saved,
                     int stop_at_input) {
  const clipfs_tower* t = p.t;
  CLIPFS_CHECK(check_bwd_weights(t));
  const int seq = t->seq, d = t->width, top = t->layers - 1;
  if (!rows) return bwd_walk(p, dx, saved, stop_at_input, top);
  if (!last_block_rows_ok(t)) {  // dense fall-back: the row gradients scattered into zeros
    CLIPFS_CHECK(clipfs_scatter_rows(dxs, rows, dx, p.batch, seq, d, p.st));
    return bwd_walk(p, dx, saved, stop_at_input, top);
  }
  const float* sv = saved + (size_t)(top - t->grad_lo) * p.SL.total;
  float *dxm_s, *datt_s;
  CLIPFS_CHECK(bwd_head(p, sv, dxs, rows, &dxm_s, &datt_s));
  // attention and the QKV projection see every row of the view again
  float* datt = p.scratch + p.SC.b1;
  if (p.v.packed()) {
    // datt and dx (the residual around the attention) are zero except at the EOT rows.  Put before the lower half
    // gathers anything into the MLP scratch that holds datt_s / dxm_s.
    float* dxw = packed_x(p);
    hipError_t e = hipMemsetAsync(datt, 0, ((size_t)(dxw - datt) + (size_t)p.v.n * d) * sizeof(float), p.st);
    CLIPFS_REQUIRE(e == hipSuccess, "tower_bwd_packed: memset failed: %s", hipGetErrorString(e));
    CLIPFS_CHECK(clipfs_put_rows_map(datt_s, p.v.eotp, datt, (size_t)d, p.batch, d, p.st));
    CLIPFS_CHECK(clipfs_put_rows_map(dxm_s, p.v.eotp, dxw, (size_t)d, p.batch, d, p.st));
    CLIPFS_CHECK(bwd_attn_half(p, top, sv, dxw, nullptr, nullptr, nullptr, stop_at_input));
  } else {
    // LayerNorm 1's backward writes every row of dx (no f16 image: bwd_walk makes it on entry to the blocks below)
    CLIPFS_CHECK(clipfs_scatter_rows(datt_s, rows, datt, p.batch, seq, d, p.st));
    CLIPFS_CHECK(bwd_attn_half(p, top, sv, dx, nullptr, dxm_s, rows, stop_at_input));
  }
  if (!needs_dx(t, top, stop_at_input)) return CLIPFS_OK;
  return bwd_walk(p, dx, saved, stop_at_input, top - 1);
}

extern "C" int clipfs_tower_bwd(const clipfs_tower* t, float* dx, int batch, const float* saved, float* scratch,
                                int stop_at_input, void* stream) {
  Pass p;
  CLIPFS_CHECK(begin_pass(&p, "tower_bwd", t, batch, dx && saved && scratch, &stop_at_input, nullptr, 0, scratch, stream));
  return tower_bwd(p, nullptr, nullptr, dx, saved, stop_at_input);
}

extern "C" int clipfs_tower_bwd_sparse(const clipfs_tower* t, const float* dxs, const int32_t* rows, float* dx, int batch,
                                       const float* saved, float* scratch, int stop_at_input, void* stream) {
  Pass p;
  CLIPFS_CHECK(begin_pass(&p, "tower_bwd_sparse", t, batch, dxs && rows && dx && saved && scratch, &stop_at_input, nullptr,
                          0, scratch, stream));
  return tower_bwd(p, dxs, rows, dx, saved, stop_at_input);
}

// ---- live rows of a causal tower -----------------------------------------------------------------------------------

static bool pack_dropout_ok(const clipfs_tower* t) {
  // the adapter backward must not evaluate Philox on packed rows (it would index the masks by the packed row): with
  // dropout active the q/k/v masks come from the saved keep bits, and the o-projection adapter has none
  const bool drop = t->lora_r > 0 && t->lora_dropout > 0.f && t->dropout_seed != 0;
  if (!drop) return true;
  for (int l = t->grad_lo; l < t->layers; ++l) {
    const Adapters ad = adapters(t->blocks[l]);
    if (ad.o) return false;
    if (ad.qkv_mask && !keep_bits_saved(t)) return false;
  }
  return true;
}

// Packing runs only where its buffers fit the existing scratch slots (R <= M / 2: b1 = the attention gradient | the
// residual gradient; big = du | the gathered u, then the other gathered tensors), its kernels exist and the tower is
// large enough to gain; everything else keeps the dense rows, so the scratch size does not change.
// Below kPackMinRows dense rows the text backward is launch-bound (a few captions: tens of microseconds per block) and
// the per-block gathers would cost what the smaller products save; such towers keep the dense rows and their arithmetic.
constexpr int kPackMinRows = 2048;

// fp16 storage mode packs the backward on the f16 attention kernels; the walk reads the transposed f16 planes of every
// block it visits (check_bwd_weights refuses a backward without them: a descriptor without them is no training one).
// Its gathers fit the `big` slot as the fp32 mode's do: u as halves sits behind the (unwritten) fp32 du, 4 R d + 2 R d
// <= 4 M d for R <= M / 2, and the later h1 / t_qkv / keep-bit gathers take R (2.125 d + 4 r) floats.
static bool pack_ok(const clipfs_tower* t, int batch, int R) {
  const int M = batch * t->seq, d = t->width, r = t->lora_r;
  if (M < kPackMinRows) return false;
  if (!t->causal || !last_block_rows_ok(t)) return false;
  // MLP adapters keep the dense rows in both directions: their down-projections and backward products are not carried
  // through the row map (the masks would have to be drawn at the full-layout row)
  if (tower_has_mlp_lora(t)) return false;
  switch (attn_route(t, true, false)) {  // of the live rows over dense records: is there a kernel for it?
    case AttnRoute::F16Packed:
      if (!clipfs_attention_f16_bwd_packed_ok(t->seq, 1)) return false;
      for (int l = t->grad_lo; l < t->layers; ++l) {
        const clipfs_block& b = t->blocks[l];
        if (!b.w_qkv_t_p || !b.w_o_t_p || !b.w_fc_t_p || !b.w_pr_t_p) return false;
      }
      break;
    case AttnRoute::Fp32Packed:
      if (!clipfs_attention_bwd_packed_ok(t->seq, 1)) return false;
      break;
    default: return false;  // Fp32Fallback
  }
  if (R < batch || 2 * (size_t)R > (size_t)M || (d % 8) != 0) return false;
  if (!pack_dropout_ok(t)) return false;
  const ScratchLayout SC = scratch_layout(t, (size_t)M);
  if (r > 0) {
    const size_t need = al4(clipfs_lora_bwd_work_floats(R, d, r, 3));
    if (need > SC.gemm_ws - SC.work) return false;  // the slice count is not monotone in the rows
  }
  if (tower_has_bias_slots(t)) {
    const int widths[3] = {d, 3 * d, 4 * d};
    for (int i = 0; i < 3; ++i)
      if (clipfs_bias_grad_work_floats(R, widths[i]) > SC.total - SC.bwork) return false;
  }
  return true;
}

// The live-row forward reproduces the dense one bitwise (tower_fwd), which needs the dense launches to be unsplit too
static bool pack_fwd_ok(const clipfs_tower* t, int batch, int R) {
  if (!pack_ok(t, batch, R) || t->weight_format != 0) return false;  // exact fp32 only
  const int M = batch * t->seq, d = t->width, r = t->lora_r;
  for (int i = 0; i < kFwdGemms; ++i)  // split-K at M?
    if (clipfs_gemm_workspace_floats(M, kGemmShape[i][0] * d, kGemmShape[i][1] * d) != 0) return false;
  // dropout on the packed rows: only the fused LayerNorm + down-projection draws its masks through the row map, and the
  // blocks below grad_lo draw them too
  if (r > 0 && t->lora_dropout > 0.f && t->dropout_seed != 0)
    for (int l = 0; l < t->layers; ++l) {
      const Adapters ad = adapters(t->blocks[l]);
      if (ad.o) return false;
      if (ad.qkv_mask && !clipfs_layernorm_fwd_lora_ok(d, r, 3)) return false;
    }
  return true;
}

static bool mode_query_ok(const clipfs_tower* t, int batch) {
  if (!t || !t->blocks || t->struct_size != sizeof(clipfs_tower) || t->block_size != sizeof(clipfs_block)) return false;
  return batch > 0 && t->layers > 0 && t->seq > 0 && t->grad_lo >= 0 && t->grad_lo < t->layers;
}

extern "C" int clipfs_tower_pack_mode(const clipfs_tower* t, int batch, int R) {
  return mode_query_ok(t, batch) && pack_ok(t, batch, R) ? 1 : 0;
}

extern "C" int clipfs_tower_pack_fwd_mode(const clipfs_tower* t, int batch, int R) {
  return mode_query_ok(t, batch) && pack_fwd_ok(t, batch, R) ? 1 : 0;
}

extern "C" int clipfs_tower_bwd_packed(const clipfs_tower* t, const float* dxs, const int32_t* rows, const int32_t* plan,
                                       int R, float* dx, int batch, const float* saved, float* scratch, int stop_at_input,
                                       void* stream) {
  Pass p;
  CLIPFS_CHECK(begin_pass(&p, "tower_bwd_packed", t, batch, dxs && rows && plan && dx && saved && scratch, &stop_at_input,
                          plan, R, scratch, stream));
  if (pack_ok(t, batch, R)) packed_rows(&p, false, false);  // else the dense rows (clipfs_tower_pack_mode says which)
  return tower_bwd(p, dxs, rows, dx, saved, stop_at_input);
}

extern "C" int clipfs_tower_fwd_packed(const clipfs_tower* t, float* x, const int32_t* rows, const int32_t* plan, int R,
                                       int batch, float* saved, float* scratch, void* stream) {
  Pass p;
  CLIPFS_CHECK(begin_pass(&p, "tower_fwd_packed", t, batch, x && rows && plan && scratch, nullptr, plan, R, scratch, stream));
  if (pack_fwd_ok(t, batch, R)) {  // else the dense rows (clipfs_tower_pack_fwd_mode says which)
    packed_rows(&p, true, true);
    return tower_fwd(p, x, rows, saved);
  }
  return tower_fwd(p, x, last_block_rows_ok(t) ? rows : nullptr, saved);
}

extern "C" int clipfs_tower_bwd_packed_saved(const clipfs_tower* t, const float* dxs, const int32_t* rows, const int32_t* plan,
                                             int R, float* dx, int batch, const float* saved, float* scratch, int stop_at_input,
                                             void* stream) {
  Pass p;
  CLIPFS_CHECK(begin_pass(&p, "tower_bwd_packed_saved", t, batch, dxs && rows && plan && dx && saved && scratch,
                          &stop_at_input, plan, R, scratch, stream));
  // the saved tensors must be clipfs_tower_fwd_packed's packed ones: no fall-back here
  CLIPFS_REQUIRE(pack_fwd_ok(t, batch, R), "tower_bwd_packed_saved: this geometry runs the dense forward (pack_fwd_mode 0)");
  packed_rows(&p, true, false);
  return tower_bwd(p, dxs, rows, dx, saved, stop_at_input);
}
