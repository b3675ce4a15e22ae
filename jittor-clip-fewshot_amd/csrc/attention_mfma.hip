// Exact-fp32 attention on the matrix cores (v_mfma_f32_32x32x2_f32, the instruction of the dense GEMMs): the
// function of attention.hip (jclip/mha.py:55-83,439-458), forward, dQ and dK/dV: one workgroup per head up to 288 tokens
// (below), runs of tiles against a chunked other side up to 1024 (the long kernels further down).
// Same structure as attention_f16.hip, with fp32 operands end to end (products exact in fp32, fp32 accumulate; only
// the summation order differs from the VALU kernels):
//
//   * one workgroup per (batch, head), one wave per 32-token tile of the "own" side (queries in the forward and the
//     dQ pass, keys in the dK/dV pass); the own rows sit in registers as MFMA B operands (lane = row lane & 31,
//     features 32 (lane >> 5) .. + 31: the K-slot <-> feature assignment of an MFMA sum is free as long as A and B
//     agree, so each half-wave simply takes one contiguous half of the 64 features);
//   * scores are produced TRANSPOSED (S^T[other][own] = Other Own^T), so a lane holds 16 other-side tokens of ONE
//     own token: softmax statistics are per-lane scalars (+ one exchange with lane ^ 32) and P^T / dS^T are already
//     the B operand of the token-axis product; its A operand is read from the TRANSPOSED image of the other side
//     kept in LDS ([64 features][tokens], 16-byte reads of 4 consecutive tokens);
//   * the row-major other-side tiles (A operand of the score product) are read straight from global memory /
//     L2 (each lane 128 contiguous bytes), so LDS holds only the transposed images: 26 KB per head at L = 77.
#include "common.h"

namespace clipfs {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int AM_HD = 64;
constexpr float AM_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float am_xor32(float v) { return __shfl_xor(v, 32, 64); }

// transposed fp32 image of a head's [L][64] slice: tr[f * TP + tok], TP = Lp + 4 (conflict-free ds_read_b128 for
// lanes = consecutive features); tokens [L, Lp) zero-filled.
__device__ __forceinline__ void am_stage_T(const float* __restrict__ src, size_t ld, int L, int Lp, float* tr) {
  const int TP = Lp + 4;
  for (int idx = threadIdx.x; idx < Lp * 16; idx += (int)blockDim.x) {
    const int c = idx / Lp, tok = idx - c * Lp;  // token fastest: conflict-free ds_write_b32
    f32x4 v;
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (tok < L) v = *reinterpret_cast<const f32x4*>(src + (size_t)tok * ld + 4 * c);
#pragma unroll
    for (int j = 0; j < 4; ++j) tr[(4 * c + j) * TP + tok] = v[j];
  }
}

// own rows as B operands: own[i] = row (t0 + lane & 31), feature 32 (lane >> 5) + i
__device__ __forceinline__ void am_load_own(const float* __restrict__ src, size_t ld, int t0, int L, int lane, float (&own)[32]) {
  const float* p = src + (size_t)min(t0 + (lane & 31), L - 1) * ld + 32 * (lane >> 5);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) own[4 * j + e] = v[e];
  }
}

// acc[other token t0 + reg-row][own token = lane] = sum_f other[tok][f] own[lane][f]; other rows from global memory
__device__ __forceinline__ f32x16 am_scores_T(const float* __restrict__ other, size_t ld, int t0, int L, int lane,
                                              const float (&own)[32]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* p = other + (size_t)min(t0 + (lane & 31), L - 1) * ld + 32 * (lane >> 5);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma32(v[e], own[4 * j + e], acc);
  }
  return acc;
}

// acc[feature dt*32 + reg-row][own = lane] += sum over the tile's 32 tokens of tr[feature][t0 + tok] * w[tok][own],
// w = the lane's 16 registers (tokens (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
__device__ __forceinline__ f32x16 am_accum_T(const float* tr, int TP, int dt, int t0, int lane, const f32x16& w, f32x16 acc) {
  const float* p = tr + (dt * 32 + (lane & 31)) * TP + t0 + 4 * (lane >> 5);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma32(v[e], w[4 * g + e], acc);
  }
  return acc;
}

__device__ __forceinline__ void am_store_T(float* __restrict__ dst, const f32x16 (&o)[2], float scale, int lane) {
  // lane holds features dt*32 + 8 g + 4 (lane >> 5) + {0..3} of its own row: 16-byte stores
  float* p = dst + 4 * (lane >> 5);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = o[t][4 * g + j] * scale;
      *reinterpret_cast<f32x4*>(p + 32 * t + 8 * g) = v;
    }
}

// ---- one 32-token tile of the other side, shared by the short kernels (whole head in LDS) and the long ones (the head
// passes through LDS in chunks): `k0` / `i0` is the tile's first token in the sequence (row-major rows from global memory,
// masks), `kl` / `il` the same token's column in the transposed LDS image(s) -- equal in the short kernels, minus the chunk's
// first token in the long ones.  Same operations in the same order for either caller, so a long kernel walking an own
// tile's other-side tiles in ascending order gives the short kernel's bits.
// Macros, not functions: the compiler simplifies a callee on its own before it inlines it and then builds the dK/dV tile
// differently (selects for branches: the 257-token backward measured 3 % slower), while the expanded text leaves the short
// kernels' instruction streams exactly those they had as plain loops.  Each body uses the names of the pass it belongs
// to, which both of its kernels define: q0, d, ld, L, lane, fh, c and
//   forward:  qf, klim, sVt, TP, o, m, l          (online-softmax update with keys k0 .. k0 + 31)
//   dQ:       qf, gf, klim, lse2, Di, sKt, TP, acc (acc += K^T dS^T over keys k0 .. k0 + 31)
//   dK/dV:    g0, kf, vf, k_tok, causal, sLse, sD, sQt, sGt, TP, av, ak   (av += dO^T P, ak += Q^T dS over queries i0 ..)
#define AM_FWD_TILE(k0, kl)                                   \
  do {                                                        \
    f32x16 s = am_scores_T(q0 + d, ld, (k0), L, lane, qf);    \
    float mt = -INFINITY;                                     \
    _Pragma("unroll")                                         \
    for (int r = 0; r < 16; ++r) {                            \
      const int key = (k0) + (r & 3) + 8 * (r >> 2) + 4 * fh; \
      s[r] = (key < L && key <= klim) ? s[r] * c : -INFINITY; \
      mt = fmaxf(mt, s[r]);                                   \
    }                                                         \
    mt = fmaxf(mt, am_xor32(mt));                             \
    const float mn = fmaxf(m, mt);                            \
    const float f = __builtin_amdgcn_exp2f(m - mn);           \
    float ps = 0.f;                                           \
    _Pragma("unroll")                                         \
    for (int r = 0; r < 16; ++r) {                            \
      s[r] = __builtin_amdgcn_exp2f(s[r] - mn);               \
      ps += s[r];                                             \
    }                                                         \
    l = l * f + ps;                                           \
    m = mn;                                                   \
    _Pragma("unroll")                                         \
    for (int t = 0; t < 2; ++t) {                             \
      _Pragma("unroll")                                       \
      for (int r = 0; r < 16; ++r) o[t][r] *= f;              \
      o[t] = am_accum_T(sVt, TP, t, (kl), lane, s, o[t]);     \
    }                                                         \
  } while (0)

#define AM_BWD_Q_TILE(k0, kl)                                                                   \
  do {                                                                                          \
    const f32x16 s = am_scores_T(q0 + d, ld, (k0), L, lane, qf);                                \
    const f32x16 dp = am_scores_T(q0 + 2 * d, ld, (k0), L, lane, gf);                           \
    f32x16 ds;                                                                                  \
    _Pragma("unroll")                                                                           \
    for (int r = 0; r < 16; ++r) {                                                              \
      const int key = (k0) + (r & 3) + 8 * (r >> 2) + 4 * fh;                                   \
      const float p = (key < L && key <= klim) ? __builtin_amdgcn_exp2f(s[r] * c - lse2) : 0.f; \
      ds[r] = p * (dp[r] - Di) * 0.125f;                                                        \
    }                                                                                           \
    _Pragma("unroll")                                                                           \
    for (int t = 0; t < 2; ++t) acc[t] = am_accum_T(sKt, TP, t, (kl), lane, ds, acc[t]);        \
  } while (0)

#define AM_BWD_KV_TILE(i0, il)                                                                        \
  do {                                                                                                \
    const f32x16 s = am_scores_T(q0, ld, (i0), L, lane, kf);                                          \
    const f32x16 dp = am_scores_T(g0, (size_t)d, (i0), L, lane, vf);                                  \
    f32x16 p, ds;                                                                                     \
    _Pragma("unroll")                                                                                 \
    for (int g = 0; g < 4; ++g) {                                                                     \
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(sLse + (il) + 8 * g + 4 * fh);                 \
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + (il) + 8 * g + 4 * fh);                   \
      _Pragma("unroll")                                                                               \
      for (int j = 0; j < 4; ++j) {                                                                   \
        const int r = 4 * g + j;                                                                      \
        const int qi = (i0) + 8 * g + 4 * fh + j;                                                     \
        p[r] = (qi < L && (!causal || qi >= k_tok)) ? __builtin_amdgcn_exp2f(s[r] * c - l4[j]) : 0.f; \
        ds[r] = p[r] * (dp[r] - d4[j]) * 0.125f;                                                      \
      }                                                                                               \
    }                                                                                                 \
    _Pragma("unroll")                                                                                 \
    for (int t = 0; t < 2; ++t) {                                                                     \
      av[t] = am_accum_T(sGt, TP, t, (il), lane, p, av[t]);                                           \
      ak[t] = am_accum_T(sQt, TP, t, (il), lane, ds, ak[t]);                                          \
    }                                                                                                 \
  } while (0)

// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_mfma_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                 float* __restrict__ lse, int L, int H, int causal) {
  extern __shared__ __attribute__((aligned(16))) float am_smem[];
  const int Lp = (L + 31) & ~31, TP = Lp + 4;
  float* sVt = am_smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int d = H * AM_HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * AM_HD;
  am_stage_T(q0 + 2 * d, ld, L, Lp, sVt);
  __syncthreads();
  const int fr = lane & 31, fh = lane >> 5;
  const float c = 0.125f * AM_LOG2E;
  for (int qt = wave; qt * 32 < L; qt += nw) {
    const int q_tok = qt * 32 + fr;
    float qf[32];
    am_load_own(q0, ld, qt * 32, L, lane, qf);
    f32x16 o[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int kend = causal ? min(L, qt * 32 + 32) : L;
    const int klim = causal ? q_tok : L - 1;
    for (int k0 = 0; k0 < kend; k0 += 32) AM_FWD_TILE(k0, k0);
    l += am_xor32(l);
    if (q_tok < L) {
      am_store_T(out + ((size_t)b * L + q_tok) * d + h * AM_HD, o, 1.f / l, lane);
      if (lse && fh == 0) lse[((size_t)b * H + h) * L + q_tok] = (m + log2f(l)) * (1.f / AM_LOG2E);
    }
  }
}

// dQ pass (own = queries).  S^T = K Q^T ; P^T = exp2(S^T c - lse) ; dP^T = V dO^T ; dS^T = P^T (dP^T - D) / 8 ;
// dQ^T += K^T dS^T.  Also writes D_i = dO_i . O_i for the second pass.
__global__ __launch_bounds__(256) void attention_mfma_bwd_q_kernel(const float* __restrict__ qkv,
                                                                   const float* __restrict__ dout,
                                                                   const float* __restrict__ out,
                                                                   const float* __restrict__ lse, float* __restrict__ dqkv,
                                                                   float* __restrict__ Dbuf, int L, int H, int causal) {
  extern __shared__ __attribute__((aligned(16))) float am_smem[];
  const int Lp = (L + 31) & ~31, TP = Lp + 4;
  float* sKt = am_smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int d = H * AM_HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * AM_HD;
  am_stage_T(q0 + d, ld, L, Lp, sKt);
  __syncthreads();
  const int fr = lane & 31, fh = lane >> 5;
  const float c = 0.125f * AM_LOG2E;
  for (int qt = wave; qt * 32 < L; qt += nw) {
    const int q_tok = qt * 32 + fr, q_cl = min(q_tok, L - 1);
    float qf[32], gf[32];
    am_load_own(q0, ld, qt * 32, L, lane, qf);
    am_load_own(dout + (size_t)b * L * d + (size_t)h * AM_HD, (size_t)d, qt * 32, L, lane, gf);
    float Di = 0.f;
    {
      const float* op = out + ((size_t)b * L + q_cl) * d + h * AM_HD + 32 * fh;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 ov = *reinterpret_cast<const f32x4*>(op + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) Di = fmaf(gf[4 * j + e], ov[e], Di);
      }
      Di += am_xor32(Di);
    }
    const float lse2 = lse[((size_t)b * H + h) * L + q_cl] * AM_LOG2E;
    if (q_tok < L && fh == 0) Dbuf[((size_t)b * H + h) * L + q_tok] = Di;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int kend = causal ? min(L, qt * 32 + 32) : L;
    const int klim = causal ? q_tok : L - 1;
    for (int k0 = 0; k0 < kend; k0 += 32)
      AM_BWD_Q_TILE(k0, k0);
    if (q_tok < L) am_store_T(dqkv + ((size_t)b * L + q_tok) * ld + h * AM_HD, acc, 1.f, lane);
  }
}

// dK/dV pass (own = keys).  S = Q K^T ; P = exp2(S c - lse) ; dP = dO V^T ; dS = P (dP - D) / 8 ;
// dV^T += dO^T P ; dK^T += Q^T dS.  lse and D vary with the register index (rows = queries): 4-float groups from LDS.
__global__ __launch_bounds__(256) void attention_mfma_bwd_kv_kernel(const float* __restrict__ qkv,
                                                                    const float* __restrict__ dout,
                                                                    const float* __restrict__ lse,
                                                                    const float* __restrict__ Dbuf,
                                                                    float* __restrict__ dqkv, int L, int H, int causal) {
  extern __shared__ __attribute__((aligned(16))) float am_smem[];
  const int Lp = (L + 31) & ~31, TP = Lp + 4;
  float* sQt = am_smem;
  float* sGt = sQt + 64 * TP;
  float* sLse = sGt + 64 * TP;  // [Lp], log2 units
  float* sD = sLse + Lp;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int d = H * AM_HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * AM_HD;
  const float* g0 = dout + (size_t)b * L * d + (size_t)h * AM_HD;
  am_stage_T(q0, ld, L, Lp, sQt);
  am_stage_T(g0, (size_t)d, L, Lp, sGt);
  for (int i = threadIdx.x; i < Lp; i += (int)blockDim.x) {
    sLse[i] = i < L ? lse[((size_t)b * H + h) * L + i] * AM_LOG2E : 0.f;
    sD[i] = i < L ? Dbuf[((size_t)b * H + h) * L + i] : 0.f;
  }
  __syncthreads();
  const int fr = lane & 31, fh = lane >> 5;
  const float c = 0.125f * AM_LOG2E;
  for (int kt = wave; kt * 32 < L; kt += nw) {
    const int k_tok = kt * 32 + fr;
    float kf[32], vf[32];
    am_load_own(q0 + d, ld, kt * 32, L, lane, kf);
    am_load_own(q0 + 2 * d, ld, kt * 32, L, lane, vf);
    f32x16 av[2], ak[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        av[t][r] = 0.f;
        ak[t][r] = 0.f;
      }
    for (int i0 = causal ? kt * 32 : 0; i0 < L; i0 += 32)
      AM_BWD_KV_TILE(i0, i0);
    if (k_tok < L) {
      float* kp = dqkv + ((size_t)b * L + k_tok) * ld + d + h * AM_HD;
      am_store_T(kp, ak, 1.f, lane);
      am_store_T(kp + d, av, 1.f, lane);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Long sequences, 288 < L <= AM_LONG_MAXL (ViT-L/14 at 336 px: L = 577).  The same three passes with the same tile bodies
// (AM_FWD_TILE / AM_BWD_Q_TILE / AM_BWD_KV_TILE); what changes is that neither side fits one workgroup any more:
//   * own side: the sequence's 32-token tiles are cut into `runs` equal runs of blockDim / 64 <= AM_RUN tiles, one
//     workgroup per (batch, head, run), blockIdx = (batch * H + head) * runs + run (the runs of a head are neighbours in
//     dispatch order: they read the same K / V, or Q / dO, through L2).  A wave owns ONE tile for the whole kernel, its
//     state in registers (forward: qf, o, m, l; dQ: qf, gf, Di, lse2, acc; dK/dV: kf, vf, av, ak), and every output
//     element is written by exactly one wave of one workgroup: no atomics, no cross-workgroup sums, bitwise run-to-run
//     results.  A wave walks its other-side tiles in ascending order, so its sums are those of the short kernels.
//   * other side: only the transposed image(s) live in LDS (the row-major rows come from global memory / L2), and they
//     pass through it in chunks of `ctok` <= AM_MAXL tokens (a multiple of 32), staged by am_stage_T from the chunk's
//     first token.  The dK/dV pass stages the chunk's lse and D_i values with them.  At ctok = 288 the launch asks for
//     what the short kernels ask for at L = 288 (74 752 B with one image, 151 808 B with two and the vectors), less
//     below.
// Barriers of the chunk loop: the __syncthreads() after staging orders the chunk's LDS writes before its reads (RAW);
// the one in front of the next staging orders every wave's last read of the old chunk before it is overwritten (WAR).
// Both are reached by every wave of the workgroup the same number of times: the chunk bounds depend on blockIdx and the
// launch arguments alone, and a wave with no tile (a short last run) or with nothing visible in a chunk (causal) only
// skips the tile loop.
// Causal: a run stages key chunks up to its last query (forward / dQ) or query chunks from its first key (dK/dV) only;
// a wave's visible tiles are the short kernels' (kend / i0 bounds).
// ---------------------------------------------------------------------------------------------------------
constexpr int AM_MAXL = 288;        // longest sequence of the short kernels = longest chunk
constexpr int AM_LONG_MAXL = 1024;
constexpr int AM_LONG_MINL = 97;    // below: the 16-token-tile kernels (attention_mfma16.hip)
constexpr int AM_RUN = 4;           // tiles per run: the 256 threads of the short kernels (8 would cap dK/dV at 256 registers)

__global__ __launch_bounds__(64 * AM_RUN) void attention_mfma_long_fwd_kernel(const float* __restrict__ qkv,
                                                                              float* __restrict__ out,
                                                                              float* __restrict__ lse, int L, int H,
                                                                              int causal, int runs, int ctok) {
  extern __shared__ __attribute__((aligned(16))) float am_smem[];
  float* sVt = am_smem;  // [64][chunk tokens + 4]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  const int bh = blockIdx.x / runs, run = blockIdx.x - bh * runs;
  const int b = bh / H, h = bh % H;
  const int d = H * AM_HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * AM_HD;
  const int fr = lane & 31, fh = lane >> 5;
  const float c = 0.125f * AM_LOG2E;
  const int qt = run * nw + wave;  // the wave's query tile
  const int q_tok = qt * 32 + fr;
  float qf[32];
  am_load_own(q0, ld, qt * 32, L, lane, qf);  // rows clamped to L - 1: a wave without a tile loads the last row
  f32x16 o[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int kend = qt * 32 >= L ? 0 : causal ? min(L, qt * 32 + 32) : L;  // this wave's keys (none: no tile in a short run)
  const int klim = causal ? q_tok : L - 1;
  const int kall = causal ? min(L, (run + 1) * nw * 32) : L;  // the run's keys
  for (int c0 = 0; c0 < kall; c0 += ctok) {
    const int Lc = min(ctok, kall - c0), Lpc = (Lc + 31) & ~31, TP = Lpc + 4;
    if (c0) __syncthreads();
    am_stage_T(q0 + 2 * d + (size_t)c0 * ld, ld, Lc, Lpc, sVt);
    __syncthreads();
    const int kstop = min(c0 + Lc, kend);
    for (int k0 = c0; k0 < kstop; k0 += 32) AM_FWD_TILE(k0, k0 - c0);
  }
  l += am_xor32(l);
  if (q_tok < L) {
    am_store_T(out + ((size_t)b * L + q_tok) * d + h * AM_HD, o, 1.f / l, lane);
    if (lse && fh == 0) lse[((size_t)b * H + h) * L + q_tok] = (m + log2f(l)) * (1.f / AM_LOG2E);
  }
}

// dQ (and D_i) of a long sequence: own side = the wave's query tile; K^T passes through LDS in key chunks.
__global__ __launch_bounds__(64 * AM_RUN) void attention_mfma_long_bwd_q_kernel(
    const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ out,
    const float* __restrict__ lse, float* __restrict__ dqkv, float* __restrict__ Dbuf, int L, int H, int causal, int runs,
    int ctok) {
  extern __shared__ __attribute__((aligned(16))) float am_smem[];
  float* sKt = am_smem;  // [64][chunk tokens + 4]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  const int bh = blockIdx.x / runs, run = blockIdx.x - bh * runs;
  const int b = bh / H, h = bh % H;
  const int d = H * AM_HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * AM_HD;
  const int fr = lane & 31, fh = lane >> 5;
  const float c = 0.125f * AM_LOG2E;
  const int qt = run * nw + wave;
  const int q_tok = qt * 32 + fr, q_cl = min(q_tok, L - 1);
  float qf[32], gf[32];
  am_load_own(q0, ld, qt * 32, L, lane, qf);
  am_load_own(dout + (size_t)b * L * d + (size_t)h * AM_HD, (size_t)d, qt * 32, L, lane, gf);
  float Di = 0.f;
  {
    const float* op = out + ((size_t)b * L + q_cl) * d + h * AM_HD + 32 * fh;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 ov = *reinterpret_cast<const f32x4*>(op + 4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) Di = fmaf(gf[4 * j + e], ov[e], Di);
    }
    Di += am_xor32(Di);
  }
  const float lse2 = lse[((size_t)b * H + h) * L + q_cl] * AM_LOG2E;
  if (q_tok < L && fh == 0) Dbuf[((size_t)b * H + h) * L + q_tok] = Di;
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const int kend = qt * 32 >= L ? 0 : causal ? min(L, qt * 32 + 32) : L;
  const int klim = causal ? q_tok : L - 1;
  const int kall = causal ? min(L, (run + 1) * nw * 32) : L;
  for (int c0 = 0; c0 < kall; c0 += ctok) {
    const int Lc = min(ctok, kall - c0), Lpc = (Lc + 31) & ~31, TP = Lpc + 4;
    if (c0) __syncthreads();
    am_stage_T(q0 + d + (size_t)c0 * ld, ld, Lc, Lpc, sKt);
    __syncthreads();
    const int kstop = min(c0 + Lc, kend);
    for (int k0 = c0; k0 < kstop; k0 += 32)
      AM_BWD_Q_TILE(k0, k0 - c0);
  }
  if (q_tok < L) am_store_T(dqkv + ((size_t)b * L + q_tok) * ld + h * AM_HD, acc, 1.f, lane);
}

// dK, dV of a long sequence: own side = the wave's key tile; Q^T and dO^T with the queries' lse and D_i pass through LDS in
// query chunks.
__global__ __launch_bounds__(64 * AM_RUN) void attention_mfma_long_bwd_kv_kernel(
    const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ Dbuf, float* __restrict__ dqkv, int L, int H, int causal, int runs, int ctok) {
  extern __shared__ __attribute__((aligned(16))) float am_smem[];
  float* sQt = am_smem;                 // [64][chunk tokens + 4]
  float* sGt = sQt + 64 * (ctok + 4);   // [64][chunk tokens + 4]
  float* sLse = sGt + 64 * (ctok + 4);  // [ctok], log2 units
  float* sD = sLse + ctok;              // [ctok]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  const int bh = blockIdx.x / runs, run = blockIdx.x - bh * runs;
  const int b = bh / H, h = bh % H;
  const int d = H * AM_HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * AM_HD;
  const float* g0 = dout + (size_t)b * L * d + (size_t)h * AM_HD;
  const int fr = lane & 31, fh = lane >> 5;
  const float c = 0.125f * AM_LOG2E;
  const int kt = run * nw + wave;  // the wave's key tile
  const int k_tok = kt * 32 + fr;
  float kf[32], vf[32];
  am_load_own(q0 + d, ld, kt * 32, L, lane, kf);
  am_load_own(q0 + 2 * d, ld, kt * 32, L, lane, vf);
  f32x16 av[2], ak[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      av[t][r] = 0.f;
      ak[t][r] = 0.f;
    }
  const int ibeg = kt * 32 >= L ? L : causal ? kt * 32 : 0;  // this wave's first query tile (L: no tile in a short run)
  for (int c0 = causal ? run * nw * 32 : 0; c0 < L; c0 += ctok) {  // the run's queries
    const int Lc = min(ctok, L - c0), Lpc = (Lc + 31) & ~31, TP = Lpc + 4;
    if (c0 != (causal ? run * nw * 32 : 0)) __syncthreads();
    am_stage_T(q0 + (size_t)c0 * ld, ld, Lc, Lpc, sQt);
    am_stage_T(g0 + (size_t)c0 * d, (size_t)d, Lc, Lpc, sGt);
    for (int i = threadIdx.x; i < Lpc; i += (int)blockDim.x) {
      sLse[i] = i < Lc ? lse[((size_t)b * H + h) * L + c0 + i] * AM_LOG2E : 0.f;
      sD[i] = i < Lc ? Dbuf[((size_t)b * H + h) * L + c0 + i] : 0.f;
    }
    __syncthreads();
    for (int i0 = max(c0, ibeg); i0 < c0 + Lc; i0 += 32)
      AM_BWD_KV_TILE(i0, i0 - c0);
  }
  if (k_tok < L) {
    float* kp = dqkv + ((size_t)b * L + k_tok) * ld + d + h * AM_HD;
    am_store_T(kp, ak, 1.f, lane);
    am_store_T(kp + d, av, 1.f, lane);
  }
}

// ---- host side: these families' share of the plan and their launchers (called from attention.hip) ----------------

// `images` transposed images of `tokens` (rounded up to whole tiles) + 4 pad; vectors: lse and D of the dK/dV pass
static unsigned am_lds(int tokens, int images, bool vectors) {
  const int Lp = (tokens + 31) & ~31;
  return (unsigned)(((size_t)images * 64 * (Lp + 4) + (vectors ? 2 * (size_t)Lp : 0)) * sizeof(float));
}

// launches of both families: the forward; or the dQ pass (which also writes D_i to `work`), then the dK/dV pass
static void am_launches(bool backward, unsigned grid, unsigned block, int lds_tokens, AttnPlan& p) {
  p.launches = backward ? 2 : 1;
  p.launch[0] = {grid, 1, block, am_lds(lds_tokens, 1, false)};
  if (backward) p.launch[1] = {grid, 1, block, am_lds(lds_tokens, 2, true)};
}

static void am_allow_lds(const void* kernel) {
  (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

void attention_mfma_plan(bool backward, int batch, int seq, int heads, AttnPlan& p) {
  const int tiles = (seq + 31) / 32;
  p.family = CLIPFS_ATTN_MFMA32;
  am_launches(backward, (unsigned)(batch * heads), 64u * (tiles < 4 ? tiles : 4), seq, p);
}

int attention_mfma_fwd(const AttnPlan& p, const float* qkv, float* out, float* lse, int seq, int heads, int causal,
                       hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    am_allow_lds(reinterpret_cast<const void*>(&attention_mfma_fwd_kernel));
    attr = true;
  }
  const clipfs_attention_launch& l = p.launch[0];
  hipLaunchKernelGGL(attention_mfma_fwd_kernel, dim3(l.grid_x), dim3(l.block), l.lds_bytes, st, qkv, out, lse, seq, heads,
                     causal);
  return launch_status();
}

int attention_mfma_bwd(const AttnPlan& p, const float* qkv, const float* dout, const float* out, const float* lse,
                       float* dqkv, float* work, int seq, int heads, int causal, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    am_allow_lds(reinterpret_cast<const void*>(&attention_mfma_bwd_q_kernel));
    am_allow_lds(reinterpret_cast<const void*>(&attention_mfma_bwd_kv_kernel));
    attr = true;
  }
  const clipfs_attention_launch &q = p.launch[0], &kv = p.launch[1];
  hipLaunchKernelGGL(attention_mfma_bwd_q_kernel, dim3(q.grid_x), dim3(q.block), q.lds_bytes, st, qkv, dout, out, lse, dqkv,
                     work, seq, heads, causal);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(attention_mfma_bwd_kv_kernel, dim3(kv.grid_x), dim3(kv.block), kv.lds_bytes, st, qkv, dout, lse, work,
                     dqkv, seq, heads, causal);
  return launch_status();
}

// the sequence's 32-token tiles cut into `parts` equal pieces of `tiles` <= max_tiles (the last may be shorter, never empty)
struct AmCut {
  int parts, tiles;
};
static AmCut am_cut(int seq, int max_tiles) {
  const int tiles = (seq + 31) / 32, parts = (tiles + max_tiles - 1) / max_tiles;
  return {parts, (tiles + parts - 1) / parts};
}

// The plan of a long launch.  chunk_tokens / run_tiles == 0: the default policy (chunks of at most AM_MAXL tokens, runs of
// at most AM_RUN tiles); either is then evened out over the sequence (577 tokens: 224 + 224 + 129, runs of 4 + 4 + 4 + 4 + 3).
int attention_mfma_long_plan(const char* what, bool backward, int batch, int seq, int heads, int chunk_tokens, int run_tiles,
                             AttnPlan& p) {
  CLIPFS_REQUIRE(batch > 0 && heads > 0, "%s: batch %d heads %d unsupported", what, batch, heads);
  CLIPFS_REQUIRE(seq >= AM_LONG_MINL && seq <= AM_LONG_MAXL, "%s: seq %d outside %d..%d", what, seq, AM_LONG_MINL,
                 AM_LONG_MAXL);
  CLIPFS_REQUIRE(chunk_tokens >= 0 && chunk_tokens <= AM_MAXL && chunk_tokens % 32 == 0,
                 "%s: chunk_tokens %d is not 0 or a multiple of 32 up to %d", what, chunk_tokens, AM_MAXL);
  CLIPFS_REQUIRE(run_tiles >= 0 && run_tiles <= AM_RUN, "%s: run_tiles %d outside 0..%d", what, run_tiles, AM_RUN);
  const AmCut own = am_cut(seq, run_tiles ? run_tiles : AM_RUN);
  CLIPFS_REQUIRE((long long)batch * heads * own.parts <= 0x7fffffffLL, "%s: batch %d x heads %d too large for seq %d", what,
                 batch, heads, seq);
  p = AttnPlan{};
  p.family = CLIPFS_ATTN_MFMA_LONG;
  p.parts = own.parts;
  p.tiles = own.tiles;
  p.ctok = 32 * am_cut(seq, (chunk_tokens ? chunk_tokens : AM_MAXL) / 32).tiles;
  am_launches(backward, (unsigned)(batch * heads * own.parts), 64u * own.tiles, p.ctok, p);
  return CLIPFS_OK;
}

int attention_mfma_long_fwd(const AttnPlan& p, const float* qkv, float* out, float* lse, int seq, int heads, int causal,
                            hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    am_allow_lds(reinterpret_cast<const void*>(&attention_mfma_long_fwd_kernel));
    attr = true;
  }
  const clipfs_attention_launch& l = p.launch[0];
  hipLaunchKernelGGL(attention_mfma_long_fwd_kernel, dim3(l.grid_x), dim3(l.block), l.lds_bytes, st, qkv, out, lse, seq, heads,
                     causal, p.parts, p.ctok);
  return launch_status();
}

int attention_mfma_long_bwd(const AttnPlan& p, const float* qkv, const float* dout, const float* out, const float* lse,
                            float* dqkv, float* work, int seq, int heads, int causal, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    am_allow_lds(reinterpret_cast<const void*>(&attention_mfma_long_bwd_q_kernel));
    am_allow_lds(reinterpret_cast<const void*>(&attention_mfma_long_bwd_kv_kernel));
    attr = true;
  }
  const clipfs_attention_launch &q = p.launch[0], &kv = p.launch[1];
  hipLaunchKernelGGL(attention_mfma_long_bwd_q_kernel, dim3(q.grid_x), dim3(q.block), q.lds_bytes, st, qkv, dout, out, lse,
                     dqkv, work, seq, heads, causal, p.parts, p.ctok);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(attention_mfma_long_bwd_kv_kernel, dim3(kv.grid_x), dim3(kv.block), kv.lds_bytes, st, qkv, dout, lse, work,
                     dqkv, seq, heads, causal, p.parts, p.ctok);
  return launch_status();
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_attention_mfma_max_seq(void) { return AM_LONG_MAXL; }

// the long kernels with an explicit cut: their own plan, their own pointer checks
extern "C" int clipfs_attention_mfma_long_fwd(const float* qkv, float* out, float* lse, int batch, int seq, int heads,
                                              int causal, int chunk_tokens, int run_tiles, void* stream) {
  AttnPlan p;
  CLIPFS_CHECK(attention_mfma_long_plan("attention_mfma_long_fwd", false, batch, seq, heads, chunk_tokens, run_tiles, p));
  CLIPFS_REQUIRE(qkv && out, "attention_mfma_long_fwd: null qkv or out");
  CLIPFS_REQUIRE(aligned16(qkv) && aligned16(out), "attention_mfma_long_fwd: misaligned pointer");
  return attention_mfma_long_fwd(p, qkv, out, lse, seq, heads, causal, (hipStream_t)stream);
}

extern "C" int clipfs_attention_mfma_long_bwd(const float* qkv, const float* dout, const float* out, const float* lse,
                                              float* dqkv, float* work, int batch, int seq, int heads, int causal,
                                              int chunk_tokens, int run_tiles, void* stream) {
  AttnPlan p;
  CLIPFS_CHECK(attention_mfma_long_plan("attention_mfma_long_bwd", true, batch, seq, heads, chunk_tokens, run_tiles, p));
  CLIPFS_REQUIRE(qkv && dout && out && lse && dqkv && work, "attention_mfma_long_bwd: null qkv, dout, out, lse, dqkv or work");
  CLIPFS_REQUIRE(aligned16(qkv) && aligned16(dout) && aligned16(out) && aligned16(dqkv),
                 "attention_mfma_long_bwd: misaligned pointer");
  return attention_mfma_long_bwd(p, qkv, dout, out, lse, dqkv, work, seq, heads, causal, (hipStream_t)stream);
}
