// Exact-fp32 self-attention for head_dim 64: the ONE dispatch plan of clipfs_attention_fwd / _bwd and their packed
// (live-row) forms, and the VALU kernels that take what the matrix-core kernels decline.
//
// The path is on the matrix cores: 16-token tiles up to 96 tokens (attention_mfma16.hip), 32-token tiles up to 288 and
// runs of tiles against a chunked other side up to 1024 (attention_mfma.hip).  attention_plan() below is the only place
// that chooses between them: direction, seq, causal, flags -> kernel family, launches, grid, block, dynamic LDS.  The
// entry points execute that plan, clipfs_attention_plan() returns it without opening a GPU, and
// tests/test_attention_plan.py pins it.  Each kernel file states the geometry of its own family (attention16_plan,
// attention_mfma_plan, attention_mfma_long_plan); nothing outside attention_plan() decides a family.
//
// The kernels of this file:
//   * attention_generic_*: one wave per query (forward, dQ) or key (dK, dV) row, the other side streamed from L2 in
//     blocks of 64 with an online softmax.  Correct for any length and any alignment of out / dqkv, not tuned: the
//     fallback for seq > 1024, a misaligned out / dqkv, and CLIPFS_ATTN_MFMA=0.
//   * attention_bwd_kernel<LMAX>: one workgroup per (batch, head), seq <= 96, recomputes the softmax from q and k:
//     the backward of a caller that did not keep the forward's out / lse.  Every inner loop is
//     FMA(register operand, broadcast operand): "row" operands (lane = key) and "column" operands (lane = feature)
//     live in VGPRs, the broadcast operand is a wave-uniform global row or a vector parked in LDS and read back 4 at
//     a time with one same-address ds_read_b128; softmax max / sum are DPP wave reductions (common.h).
// The [L, L] matrices of the reference (jclip/mha.py:79-83: a 30-77 MB HBM round trip per layer) never leave the chip,
// and heads are merged by the store address (no permute pass, mha.py:458).
#include "common.h"

#include <stdlib.h>

namespace clipfs {

constexpr int HD = 64;
constexpr int KSTRIDE = 68;  // staged K/V row stride (floats): 16-byte aligned, conflict-free ds_read_b128 by row

typedef float f32x4 __attribute__((ext_vector_type(4)));

// cooperative copy of L rows of 64 floats (global row stride ld) into LDS rows of KSTRIDE floats
__device__ __forceinline__ void stage_rows(const float* __restrict__ base, size_t ld, float* __restrict__ dst, int L,
                                           int tid) {
  for (int idx = tid; idx < L * (HD / 4); idx += (int)blockDim.x) {
    const int r = idx >> 4, c = idx & 15;
    *reinterpret_cast<f32x4*>(dst + r * KSTRIDE + 4 * c) = *reinterpret_cast<const f32x4*>(base + (size_t)r * ld + 4 * c);
  }
}

// lane j takes row j (+64 per kk) of a staged [L][KSTRIDE] image into registers; rows >= L are zero
template <int KPL>
__device__ __forceinline__ void rows_to_regs(const float* __restrict__ s, int lane, int L, float (&reg)[KPL][HD]) {
#pragma unroll
  for (int kk = 0; kk < KPL; ++kk) {
    const int j = lane + 64 * kk;
    const bool ok = j < L;
    const float* row = s + (ok ? j : 0) * KSTRIDE;
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
      reg[kk][4 * c + 0] = ok ? v[0] : 0.f;
      reg[kk][4 * c + 1] = ok ? v[1] : 0.f;
      reg[kk][4 * c + 2] = ok ? v[2] : 0.f;
      reg[kk][4 * c + 3] = ok ? v[3] : 0.f;
    }
  }
}

// lane d takes column d of L global rows (coalesced 256-byte row reads); entries >= L are zero
template <int LMAX>
__device__ __forceinline__ void col_to_regs(const float* __restrict__ base, size_t ld, int lane, int L,
                                            float (&reg)[LMAX]) {
  // unconditional (row-clamped) loads so all of them are in flight together; zero-select afterwards
#pragma unroll
  for (int j = 0; j < LMAX; ++j) reg[j] = base[(size_t)min(j, L - 1) * ld + lane];
#pragma unroll
  for (int j = 0; j < LMAX; ++j) reg[j] = j < L ? reg[j] : 0.f;
}

// dot of the wave-uniform global row `u` (64 floats) with each of this lane's register rows
// (`nkeys` = number of keys that are not masked for this row: key blocks of 64 beyond it are skipped)
template <int KPL>
__device__ __forceinline__ void dot_rows(const float* __restrict__ u, const float (&reg)[KPL][HD], float (&out)[KPL],
                                         int nkeys = 64 * KPL) {
  f32x4 q[HD / 4];
#pragma unroll
  for (int c = 0; c < HD / 4; ++c) q[c] = *reinterpret_cast<const f32x4*>(u + 4 * c);  // same address in every lane
#pragma unroll
  for (int kk = 0; kk < KPL; ++kk) {
    float a0 = 0.f, a1 = 0.f;
    if (64 * kk < nkeys) {  // wave-uniform
#pragma unroll
      for (int c = 0; c < HD / 4; ++c) {
        a0 = fmaf(q[c][0], reg[kk][4 * c + 0], a0);
        a1 = fmaf(q[c][1], reg[kk][4 * c + 1], a1);
        a0 = fmaf(q[c][2], reg[kk][4 * c + 2], a0);
        a1 = fmaf(q[c][3], reg[kk][4 * c + 3], a1);
      }
    }
    out[kk] = a0 + a1;
  }
}

// scores -> probabilities for query row i (lane = key): scale after the dot (mha.py:79), mask, softmax
template <int KPL>
__device__ __forceinline__ void softmax_row(float (&s)[KPL], int i, int lane, int L, int causal) {
  float m = -INFINITY;
#pragma unroll
  for (int kk = 0; kk < KPL; ++kk) {
    const int j = lane + 64 * kk;
    s[kk] *= 0.125f;
    if (j >= L || (causal && j > i)) s[kk] = -INFINITY;
    m = fmaxf(m, s[kk]);
  }
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int kk = 0; kk < KPL; ++kk) {
    s[kk] = __expf(s[kk] - m);  // exp(-inf) = 0 for masked keys
    sum += s[kk];
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int kk = 0; kk < KPL; ++kk) s[kk] = s[kk] / sum;
}

// sum_j vec[j] * col[j] for j < n: vec = 16-byte aligned LDS vector read as same-address b128 broadcasts.
// Guarded in groups of 16 (4 reads in flight per group); vec must be finite up to the group boundary and
// col[j >= L] == 0, so the overhang contributes exact zeros.
template <int LMAX>
__device__ __forceinline__ float bcast_dot(const float* __restrict__ vec, const float (&col)[LMAX], int n, int lo = 0) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int g = 0; g < LMAX / 16; ++g) {
    if (16 * g < n && 16 * g + 16 > lo) {  // entries below lo are exact zeros (causal mask) in vec
      f32x4 p[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) p[t] = *reinterpret_cast<const f32x4*>(vec + 16 * g + 4 * t);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a0 = fmaf(p[t][0], col[16 * g + 4 * t + 0], a0);
        a1 = fmaf(p[t][1], col[16 * g + 4 * t + 1], a1);
        a2 = fmaf(p[t][2], col[16 * g + 4 * t + 2], a2);
        a3 = fmaf(p[t][3], col[16 * g + 4 * t + 3], a3);
      }
    }
  }
  return (a0 + a1) + (a2 + a3);
}

// Backward: dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO, dS = P * (dP - rowsum(P * dP)), dP = dO V^T.
// P is recomputed (phase A1), never stored in HBM.  Phases (register sets are reused between phases):
//   A1  lane = key, K rows in VGPRs : P_i  -> LDS P^T[j][i]
//   A2  lane = key, V rows in VGPRs : dP_i, dS_i -> LDS dS^T[j][i] and dS[i][j]   (scale folded into dS)
//   C1  lane = d, dO and Q columns in VGPRs, per key j : dV[j], dK[j]  (P^T[j][:], dS^T[j][:] broadcast)
//   C2  lane = d, K column in VGPRs, per query i      : dQ[i]         (dS[i][:] broadcast)
template <int LMAX>
__global__ __launch_bounds__(512) void attention_bwd_kernel(const float* __restrict__ qkv,
                                                            const float* __restrict__ dout,
                                                            float* __restrict__ dqkv, int L, int H, int causal, int LP) {
  constexpr int KPL = (LMAX + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sPT = smem;              // [L][LP]  P^T
  float* sdST = sPT + L * LP;     // [L][LP]  dS^T
  float* sdS = sdST + L * LP;     // [L][LP]  dS   (aliases the staging buffer below: LP >= KSTRIDE is not needed,
  float* sKV = sdS;               //  [L][KSTRIDE] staged K rows, then V rows -- dead before dS is written)
  const int NW = (int)blockDim.x >> 6;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int d = H * HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * HD;
  const float* do0 = dout + (size_t)b * L * d + (size_t)h * HD;
  float* dq0 = dqkv + (size_t)b * L * ld + (size_t)h * HD;
  for (int idx = tid; idx < 2 * L * LP; idx += (int)blockDim.x) smem[idx] = 0.f;  // P^T, dS^T: finite zero padding
  stage_rows(q0 + d, ld, sKV, L, tid);
  __syncthreads();
  {
    float rows[KPL][HD];
    rows_to_regs<KPL>(sKV, lane, L, rows);  // K rows
    __syncthreads();
    stage_rows(q0 + 2 * d, ld, sKV, L, tid);  // V rows replace K rows in the staging buffer
    // A1: probabilities
    for (int i = wave; i < L; i += NW) {
      float s[KPL];
      dot_rows<KPL>(q0 + (size_t)i * ld, rows, s, causal ? i + 1 : L);
      softmax_row<KPL>(s, i, lane, L, causal);
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) {
        const int j = lane + 64 * kk;
        if (j < L) sPT[j * LP + i] = s[kk];
      }
    }
    __syncthreads();
    rows_to_regs<KPL>(sKV, lane, L, rows);  // V rows
    __syncthreads();                         // staging buffer is dead from here: it becomes dS
    for (int idx = tid; idx < L * LP; idx += (int)blockDim.x) sdS[idx] = 0.f;
    __syncthreads();
    // A2: dP, dS
    for (int i = wave; i < L; i += NW) {
      float dp[KPL], pv[KPL];
      dot_rows<KPL>(do0 + (size_t)i * d, rows, dp, causal ? i + 1 : L);
      float rs = 0.f;
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) {
        const int j = lane + 64 * kk;
        pv[kk] = j < L ? sPT[j * LP + i] : 0.f;
        rs = fmaf(pv[kk], dp[kk], rs);
      }
      rs = wave_sum(rs);
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) {
        const int j = lane + 64 * kk;
        const float ds = pv[kk] * (dp[kk] - rs) * 0.125f;
        if (j < L) {
          sdST[j * LP + i] = ds;
          sdS[i * LP + j] = ds;
        }
      }
    }
  }
  __syncthreads();
  {
    // C1: dV[j] = sum_i P_ij dO_i , dK[j] = sum_i dS_ij Q_i
    float doc[LMAX], qc[LMAX];
    col_to_regs<LMAX>(do0, (size_t)d, lane, L, doc);
    col_to_regs<LMAX>(q0, ld, lane, L, qc);
    for (int j = wave; j < L; j += NW) {
      const int lo = causal ? j : 0;  // P_ij = dS_ij = 0 for i < j
      const float av = bcast_dot<LMAX>(sPT + j * LP, doc, L, lo);
      const float ak = bcast_dot<LMAX>(sdST + j * LP, qc, L, lo);
      dq0[(size_t)j * ld + 2 * d + lane] = av;
      dq0[(size_t)j * ld + d + lane] = ak;
    }
  }
  {
    // C2: dQ[i] = sum_j dS_ij K_j
    float kc[LMAX];
    col_to_regs<LMAX>(q0 + d, ld, lane, L, kc);
    for (int i = wave; i < L; i += NW) dq0[(size_t)i * ld + lane] = bcast_dot<LMAX>(sdS + i * LP, kc, causal ? i + 1 : L);
  }
}


// ---------------------------------------------------------------------------------------------------------
// The streaming kernels: key (or query) blocks of 64 come from L2 with an online softmax -- one wave per query row
// (forward, dQ) or per key row (dK, dV).  Correct for any L and any alignment of out / dqkv; not tuned (no default plan
// of the project's towers returns them).  lse[(b*H + h)*L + i] = max_i + log(sum_i) of the scaled scores is written by
// the forward when it is given the buffer and reused by the backward.
// ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float dot64_row(const f32x4 (&u)[HD / 4], const float* __restrict__ row) {
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int c = 0; c < HD / 4; ++c) {
    const f32x4 k = *reinterpret_cast<const f32x4*>(row + 4 * c);
    a0 = fmaf(u[c][0], k[0], a0);
    a1 = fmaf(u[c][1], k[1], a1);
    a0 = fmaf(u[c][2], k[2], a0);
    a1 = fmaf(u[c][3], k[3], a1);
  }
  return a0 + a1;
}

// acc[lane] += sum_{t < n} vec[t] * base[(j0 + t) * ld + lane]   (vec: the wave's LDS row of 64 broadcast values)
__device__ __forceinline__ float axpy_block(const float* __restrict__ vec, const float* __restrict__ base, size_t ld,
                                            int lane, int n, float acc) {
  for (int t = 0; t < n; t += 4) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(vec + t);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (t + e < n) acc = fmaf(p[e], base[(size_t)(t + e) * ld + lane], acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void attention_generic_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                    float* __restrict__ lse, int L, int H, int causal) {
  __shared__ __attribute__((aligned(16))) float sP[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int i = blockIdx.y * 4 + wave;
  if (i >= L) return;
  const int d = H * HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * HD;
  f32x4 q[HD / 4];
#pragma unroll
  for (int c = 0; c < HD / 4; ++c) q[c] = *reinterpret_cast<const f32x4*>(q0 + (size_t)i * ld + 4 * c);
  float m = -INFINITY, l = 0.f, o = 0.f;
  const int jend = causal ? i + 1 : L;
  for (int j0 = 0; j0 < jend; j0 += 64) {
    const int j = j0 + lane;
    float s = -INFINITY;
    if (j < jend) s = dot64_row(q, q0 + d + (size_t)j * ld) * 0.125f;
    const float mn = fmaxf(m, wave_max(s));
    const float pj = __expf(s - mn);  // 0 for masked lanes
    const float f = __expf(m - mn);   // 0 on the first block (m = -inf)
    l = l * f + wave_sum(pj);
    sP[wave][lane] = pj;
    __builtin_amdgcn_wave_barrier();
    o = axpy_block(sP[wave], q0 + 2 * d + (size_t)j0 * ld, ld, lane, min(64, jend - j0), o * f);
    __builtin_amdgcn_wave_barrier();
    m = mn;
  }
  out[((size_t)b * L + i) * d + h * HD + lane] = o / l;
  if (lse && lane == 0) lse[((size_t)b * H + h) * L + i] = m + __logf(l);
}

// dQ and D_i = dO_i . O_i   (one wave per query row)
__global__ __launch_bounds__(256) void attention_generic_bwd_q_kernel(const float* __restrict__ qkv,
                                                                      const float* __restrict__ dout,
                                                                      const float* __restrict__ out,
                                                                      const float* __restrict__ lse,
                                                                      float* __restrict__ dqkv, float* __restrict__ Dbuf,
                                                                      int L, int H, int causal) {
  __shared__ __attribute__((aligned(16))) float sP[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int i = blockIdx.y * 4 + wave;
  if (i >= L) return;
  const int d = H * HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * HD;
  const float* do_i = dout + ((size_t)b * L + i) * d + h * HD;
  f32x4 q[HD / 4], g[HD / 4];
#pragma unroll
  for (int c = 0; c < HD / 4; ++c) {
    q[c] = *reinterpret_cast<const f32x4*>(q0 + (size_t)i * ld + 4 * c);
    g[c] = *reinterpret_cast<const f32x4*>(do_i + 4 * c);
  }
  const float Di = wave_sum(do_i[lane] * out[((size_t)b * L + i) * d + h * HD + lane]);
  const float li = lse[((size_t)b * H + h) * L + i];
  if (lane == 0) Dbuf[((size_t)b * H + h) * L + i] = Di;
  float acc = 0.f;
  const int jend = causal ? i + 1 : L;
  for (int j0 = 0; j0 < jend; j0 += 64) {
    const int j = j0 + lane;
    float ds = 0.f;
    if (j < jend) {
      const float pj = __expf(dot64_row(q, q0 + d + (size_t)j * ld) * 0.125f - li);
      const float dp = dot64_row(g, q0 + 2 * d + (size_t)j * ld);
      ds = pj * (dp - Di) * 0.125f;
    }
    sP[wave][lane] = ds;
    __builtin_amdgcn_wave_barrier();
    acc = axpy_block(sP[wave], q0 + d + (size_t)j0 * ld, ld, lane, min(64, jend - j0), acc);
    __builtin_amdgcn_wave_barrier();
  }
  dqkv[((size_t)b * L + i) * ld + h * HD + lane] = acc;
}

// dK and dV   (one wave per key row; queries streamed in blocks of 64, lane = query)
__global__ __launch_bounds__(256) void attention_generic_bwd_kv_kernel(const float* __restrict__ qkv,
                                                                       const float* __restrict__ dout,
                                                                       const float* __restrict__ lse,
                                                                       const float* __restrict__ Dbuf,
                                                                       float* __restrict__ dqkv, int L, int H, int causal) {
  __shared__ __attribute__((aligned(16))) float sP[4][64];
  __shared__ __attribute__((aligned(16))) float sS[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int j = blockIdx.y * 4 + wave;
  if (j >= L) return;
  const int d = H * HD;
  const size_t ld = (size_t)3 * d;
  const float* q0 = qkv + (size_t)b * L * ld + (size_t)h * HD;
  const float* do0 = dout + (size_t)b * L * d + (size_t)h * HD;
  f32x4 k[HD / 4], v[HD / 4];
#pragma unroll
  for (int c = 0; c < HD / 4; ++c) {
    k[c] = *reinterpret_cast<const f32x4*>(q0 + d + (size_t)j * ld + 4 * c);
    v[c] = *reinterpret_cast<const f32x4*>(q0 + 2 * d + (size_t)j * ld + 4 * c);
  }
  float av = 0.f, ak = 0.f;
  const int ibeg = causal ? j : 0;  // P_ij = 0 for i < j
  for (int i0 = ibeg & ~63; i0 < L; i0 += 64) {
    const int i = i0 + lane;
    float pj = 0.f, ds = 0.f;
    if (i < L && i >= ibeg) {
      const size_t st = ((size_t)b * H + h) * L + i;
      pj = __expf(dot64_row(k, q0 + (size_t)i * ld) * 0.125f - lse[st]);
      const float dp = dot64_row(v, do0 + (size_t)i * d);
      ds = pj * (dp - Dbuf[st]) * 0.125f;
    }
    sP[wave][lane] = pj;
    sS[wave][lane] = ds;
    __builtin_amdgcn_wave_barrier();
    const int n = min(64, L - i0);
    av = axpy_block(sP[wave], do0 + (size_t)i0 * d, (size_t)d, lane, n, av);
    ak = axpy_block(sS[wave], q0 + (size_t)i0 * ld, ld, lane, n, ak);
    __builtin_amdgcn_wave_barrier();
  }
  dqkv[((size_t)b * L + j) * ld + 2 * d + h * HD + lane] = av;
  dqkv[((size_t)b * L + j) * ld + d + h * HD + lane] = ak;
}

// ---- the kernel files' share of the plan and their launchers ------------------------------------------------------
// attention_mfma16.hip: 16-token tiles (seq <= 96), dense / packed / pinned (family = CLIPFS_ATTN_MFMA16*)
void attention16_plan(int family, bool backward, int batch, int seq, int heads, AttnPlan& p);
int attention16_fwd(const AttnPlan& p, const float* qkv, float* out, float* lse, const int32_t* off, int seq, int heads,
                    int causal, hipStream_t st);
int attention16_bwd(const AttnPlan& p, const float* qkv, const float* dout, const float* out, const float* lse, float* dqkv,
                    const int32_t* off, int seq, int heads, int causal, hipStream_t st);
// attention_mfma.hip: 32-token tiles, one workgroup per head (seq <= 288) ...
void attention_mfma_plan(bool backward, int batch, int seq, int heads, AttnPlan& p);
int attention_mfma_fwd(const AttnPlan& p, const float* qkv, float* out, float* lse, int seq, int heads, int causal,
                       hipStream_t st);
int attention_mfma_bwd(const AttnPlan& p, const float* qkv, const float* dout, const float* out, const float* lse,
                       float* dqkv, float* work, int seq, int heads, int causal, hipStream_t st);
// ... and the long form (seq <= clipfs_attention_mfma_max_seq()); chunk_tokens = run_tiles = 0: the default cut
int attention_mfma_long_plan(const char* what, bool backward, int batch, int seq, int heads, int chunk_tokens, int run_tiles,
                             AttnPlan& p);
int attention_mfma_long_fwd(const AttnPlan& p, const float* qkv, float* out, float* lse, int seq, int heads, int causal,
                            hipStream_t st);
int attention_mfma_long_bwd(const AttnPlan& p, const float* qkv, const float* dout, const float* out, const float* lse,
                            float* dqkv, float* work, int seq, int heads, int causal, hipStream_t st);

constexpr int ATTN16_MAX = 96;      // 16-token tiles; also the longest sequence of the recomputing backward
constexpr int ATTN_MFMA_MAX = 288;  // 32-token tiles with the other side whole in LDS
constexpr int ATTN_MAX_SEQ = 4096;

// padded row length of the recomputing backward's LDS [L][LP] matrices: >= L rounded up to 4 (b128 broadcast reads),
// LP / 4 odd so the transposed (stride-LP) writes spread over 8 distinct bank groups
static int padded_lp(int seq) {
  int lp = (seq + 3) & ~3;
  if (((lp >> 2) & 1) == 0) lp += 4;
  return lp;
}

// A/B aids, read once per process (never per launch: one rank's step is nearly host-bound).  "0" switches off.
static bool aid_on(const char* name) {
  const char* v = getenv(name);
  return !v || atoi(v) != 0;
}

static const char* const kDirName[] = {"attention_fwd", "attention_bwd", "attention_fwd_packed", "attention_bwd_packed",
                                       "attention_bwd_packed_io"};

// THE dispatch.  Pure host arithmetic: no HIP call, no state beyond the two aids.  flags: CLIPFS_ATTN_STATS (forward: lse
// was asked for -- it changes nothing, every forward kernel only guards one store with it; backward: the forward's out
// and lse and a work buffer are there) and CLIPFS_ATTN_ALIGNED (out / dqkv are 16-byte aligned).
static int attention_plan(int dir, int batch, int seq, int heads, int causal, int flags, AttnPlan& p) {
  static const bool use_mfma = aid_on("CLIPFS_ATTN_MFMA");  // 0: the streaming kernels at every length
  static const bool use_16 = aid_on("CLIPFS_ATTN16");       // 0: 32-token tiles below 97 tokens as well
  CLIPFS_REQUIRE(dir >= CLIPFS_ATTN_FWD && dir <= CLIPFS_ATTN_BWD_PACKED_IO, "attention_plan: direction %d unknown", dir);
  const char* what = kDirName[dir];
  CLIPFS_REQUIRE(batch > 0 && heads > 0 && seq > 0 && seq <= ATTN_MAX_SEQ, "%s: batch %d seq %d heads %d unsupported (seq <= %d)",
                 what, batch, seq, heads, ATTN_MAX_SEQ);
  const bool backward = dir != CLIPFS_ATTN_FWD && dir != CLIPFS_ATTN_FWD_PACKED;
  const bool stats = (flags & CLIPFS_ATTN_STATS) != 0, aligned = (flags & CLIPFS_ATTN_ALIGNED) != 0;
  const bool tiles16 = use_mfma && use_16 && seq <= ATTN16_MAX;
  p = AttnPlan{};
  if (dir >= CLIPFS_ATTN_FWD_PACKED) {  // live rows: the causal 16-token-tile kernels or nothing
    CLIPFS_REQUIRE(causal && tiles16, "%s: seq %d%s has no packed kernel", what, seq, causal ? "" : " without the causal mask");
    CLIPFS_REQUIRE(!backward || stats, "%s: null pointer (out and lse of the forward are needed)", what);
    CLIPFS_REQUIRE(aligned, "%s: misaligned pointer", what);
    attention16_plan(dir == CLIPFS_ATTN_BWD_PACKED_IO ? CLIPFS_ATTN_MFMA16_PINNED : CLIPFS_ATTN_MFMA16_PACKED, backward, batch,
                     seq, heads, p);
    return CLIPFS_OK;
  }
  if (use_mfma && aligned && (stats || !backward) && seq <= clipfs_attention_mfma_max_seq()) {
    if (tiles16)
      attention16_plan(CLIPFS_ATTN_MFMA16, backward, batch, seq, heads, p);
    else if (seq <= ATTN_MFMA_MAX)
      attention_mfma_plan(backward, batch, seq, heads, p);
    else
      CLIPFS_CHECK(attention_mfma_long_plan(what, backward, batch, seq, heads, 0, 0, p));
    return CLIPFS_OK;
  }
  const unsigned items = (unsigned)(batch * heads);
  if (stats || !backward) {  // everything else with statistics (or a forward): the streaming kernels
    p.family = CLIPFS_ATTN_STREAM;
    p.launches = backward ? 2 : 1;  // backward: dQ and D_i, then dK and dV
    p.launch[0] = p.launch[1] = {items, (unsigned)(seq + 3) / 4, 256, 0};
    return CLIPFS_OK;
  }
  CLIPFS_REQUIRE(seq <= ATTN16_MAX, "%s: seq %d > %d needs the forward's out and lse and a work buffer", what, seq, ATTN16_MAX);
  const int lp = padded_lp(seq);
  // P^T, dS^T, and dS (whose storage first serves as the [seq][KSTRIDE] K/V staging buffer) + 16 floats overhang
  const size_t third = (size_t)seq * (lp > KSTRIDE ? lp : KSTRIDE);
  p.family = CLIPFS_ATTN_RECOMPUTE;
  p.lmax = seq <= 64 ? 64 : seq <= 80 ? 80 : 96;
  p.launches = 1;
  p.launch[0] = {items, 1, seq > 64 ? 512u : 256u, (unsigned)(((size_t)2 * seq * lp + third + 16) * sizeof(float))};
  return CLIPFS_OK;
}

template <int LMAX>
static int recompute_bwd(const AttnPlan& p, const float* qkv, const float* dout, float* dqkv, int seq, int heads, int causal,
                         hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_bwd_kernel<LMAX>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((attention_bwd_kernel<LMAX>), dim3(p.launch[0].grid_x), dim3(p.launch[0].block), p.launch[0].lds_bytes,
                     st, qkv, dout, dqkv, seq, heads, causal, padded_lp(seq));
  return launch_status();
}

// validate, make the plan, execute it.  off == NULL: the dense layout
static int run_fwd(int dir, const float* qkv, float* out, float* lse, const int32_t* off, int batch, int seq, int heads,
                   int causal, hipStream_t st) {
  AttnPlan p;
  CLIPFS_CHECK(attention_plan(dir, batch, seq, heads, causal,
                              (lse ? CLIPFS_ATTN_STATS : 0) | (aligned16(out) ? CLIPFS_ATTN_ALIGNED : 0), p));
  CLIPFS_REQUIRE(qkv && out && (off || dir == CLIPFS_ATTN_FWD), "%s: null pointer", kDirName[dir]);
  CLIPFS_REQUIRE(aligned16(qkv), "%s: misaligned pointer", kDirName[dir]);
  switch (p.family) {
    case CLIPFS_ATTN_MFMA16:
    case CLIPFS_ATTN_MFMA16_PACKED: return attention16_fwd(p, qkv, out, lse, off, seq, heads, causal, st);
    case CLIPFS_ATTN_MFMA32: return attention_mfma_fwd(p, qkv, out, lse, seq, heads, causal, st);
    case CLIPFS_ATTN_MFMA_LONG: return attention_mfma_long_fwd(p, qkv, out, lse, seq, heads, causal, st);
    default:  // CLIPFS_ATTN_STREAM
      hipLaunchKernelGGL(attention_generic_fwd_kernel, dim3(p.launch[0].grid_x, p.launch[0].grid_y), dim3(p.launch[0].block),
                         0, st, qkv, out, lse, seq, heads, causal);
      return launch_status();
  }
}

static int run_bwd(int dir, const float* qkv, const float* dout, const float* out, const float* lse, float* dqkv, float* work,
                   const int32_t* off, int batch, int seq, int heads, int causal, hipStream_t st) {
  const bool stats = out && lse && (work || dir != CLIPFS_ATTN_BWD);  // the packed kernels need no work buffer
  AttnPlan p;
  CLIPFS_CHECK(attention_plan(dir, batch, seq, heads, causal,
                              (stats ? CLIPFS_ATTN_STATS : 0) |
                                  (aligned16(out) && aligned16(dqkv) ? CLIPFS_ATTN_ALIGNED : 0), p));
  CLIPFS_REQUIRE(qkv && dout && dqkv && (off || dir == CLIPFS_ATTN_BWD), "%s: null pointer", kDirName[dir]);
  CLIPFS_REQUIRE(aligned16(qkv) && aligned16(dout), "%s: misaligned pointer", kDirName[dir]);
  switch (p.family) {
    case CLIPFS_ATTN_MFMA16:
    case CLIPFS_ATTN_MFMA16_PACKED:
    case CLIPFS_ATTN_MFMA16_PINNED: return attention16_bwd(p, qkv, dout, out, lse, dqkv, off, seq, heads, causal, st);
    case CLIPFS_ATTN_MFMA32: return attention_mfma_bwd(p, qkv, dout, out, lse, dqkv, work, seq, heads, causal, st);
    case CLIPFS_ATTN_MFMA_LONG: return attention_mfma_long_bwd(p, qkv, dout, out, lse, dqkv, work, seq, heads, causal, st);
    case CLIPFS_ATTN_STREAM: {
      const dim3 grid(p.launch[0].grid_x, p.launch[0].grid_y), block(p.launch[0].block);
      hipLaunchKernelGGL(attention_generic_bwd_q_kernel, grid, block, 0, st, qkv, dout, out, lse, dqkv, work, seq, heads,
                         causal);
      CLIPFS_CHECK(launch_status());
      hipLaunchKernelGGL(attention_generic_bwd_kv_kernel, grid, block, 0, st, qkv, dout, lse, work, dqkv, seq, heads, causal);
      return launch_status();
    }
    default:  // CLIPFS_ATTN_RECOMPUTE
      if (p.lmax == 64) return recompute_bwd<64>(p, qkv, dout, dqkv, seq, heads, causal, st);
      if (p.lmax == 80) return recompute_bwd<80>(p, qkv, dout, dqkv, seq, heads, causal, st);
      return recompute_bwd<96>(p, qkv, dout, dqkv, seq, heads, causal, st);
  }
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_attention_plan(int direction, int batch, int seq, int heads, int causal, int flags,
                                     struct clipfs_attention_plan* plan) {
  CLIPFS_REQUIRE(plan, "attention_plan: null plan");
  AttnPlan p;
  CLIPFS_CHECK(attention_plan(direction, batch, seq, heads, causal, flags, p));
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_attention_fwd(const float* qkv, float* out, float* lse, int batch, int seq, int heads, int causal,
                                    void* stream) {
  return run_fwd(CLIPFS_ATTN_FWD, qkv, out, lse, nullptr, batch, seq, heads, causal, (hipStream_t)stream);
}

extern "C" int clipfs_attention_bwd(const float* qkv, const float* dout, const float* out, const float* lse, float* dqkv,
                                    float* work, int batch, int seq, int heads, int causal, void* stream) {
  return run_bwd(CLIPFS_ATTN_BWD, qkv, dout, out, lse, dqkv, work, nullptr, batch, seq, heads, causal, (hipStream_t)stream);
}

extern "C" int clipfs_attention_bwd_packed_ok(int seq, int causal) {
  AttnPlan p;
  return attention_plan(CLIPFS_ATTN_BWD_PACKED, 1, seq, 1, causal, CLIPFS_ATTN_STATS | CLIPFS_ATTN_ALIGNED, p) == CLIPFS_OK;
}

extern "C" int clipfs_attention_fwd_packed(const float* qkv, float* out, float* lse, const int32_t* off, int batch, int seq,
                                           int heads, void* stream) {
  return run_fwd(CLIPFS_ATTN_FWD_PACKED, qkv, out, lse, off, batch, seq, heads, 1, (hipStream_t)stream);
}

extern "C" int clipfs_attention_bwd_packed(const float* qkv, const float* dout, const float* out, const float* lse,
                                           float* dqkv, const int32_t* off, int batch, int seq, int heads, void* stream) {
  return run_bwd(CLIPFS_ATTN_BWD_PACKED, qkv, dout, out, lse, dqkv, nullptr, off, batch, seq, heads, 1, (hipStream_t)stream);
}

extern "C" int clipfs_attention_bwd_packed_io(const float* qkv, const float* dout, const float* out, const float* lse,
                                              float* dqkv, const int32_t* off, int batch, int seq, int heads, void* stream) {
  return run_bwd(CLIPFS_ATTN_BWD_PACKED_IO, qkv, dout, out, lse, dqkv, nullptr, off, batch, seq, heads, 1,
                 (hipStream_t)stream);
}

// one log-sum-exp per (batch, head, query): every forward kernel writes it when it is given the buffer
extern "C" size_t clipfs_attention_lse_floats(int batch, int seq, int heads) { return (size_t)batch * heads * seq; }
