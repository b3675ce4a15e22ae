// Rank-r LoRA products on the matrix cores, exact fp32 (v_mfma_f32_16x16x4_f32: the fp32 MFMA of the dense GEMMs
// in its 16x16 shape).  Same five products, same Philox dropout stream and same results (up to summation order) as
// the one-wave-per-row kernels in lora.hip (lora_plan there says which family a call gets).  At r = 16 (cfg-5) the
// scalar kernels spend ~50 wave reductions per row; here every product is a tall-skinny MFMA GEMM whose big operand
// is read once with 16-byte loads.  Ranks 1..64 run as G = ceil(r / 16) groups of 16
// rank columns (N = 16 of the MFMA); a wave keeps all G groups' accumulators, so x or dy is still read once, and its
// dropout masks drawn once, whatever the rank.  G = 1 is the r <= 16 arithmetic in its original order.
//
//   down  t[m, s r + j]   = sum_k drop_s(x)[m, k] A[s r + j, k]          A-operand = x rows, B-operand = A rows
//   dt    dt[m, s r + j]  = scale sum_n dy[m, s w + n] B[s w + n, j]
//   dB    dB[n, j]       += scale sum_m dy[m, n] t[m, seg(n) r + j]      reduction over rows: K index = row
//   dA    dA[s r + j, k] += sum_m dt[m, s r + j] drop_s(x)[m, k]
//   dx    dx[m, k]       += sum_s dropscale_s(m, k) sum_j dt[m, s r + j] A[s r + j, k]
//
// MFMA 16x16x4 layouts: A operand lane l = A[i = l & 15][k = l >> 4], B operand lane l = B[k = l >> 4][j = l & 15],
// result lane l = D[i = 4 (l >> 4) + v][j = l & 15], v = 0..3.  The k (and, for dB/dA/dx, the column) assignment is
// free as long as both operands agree, so a lane always loads FOUR CONSECUTIVE floats (one float4 = one Philox call
// = 4 dropout multipliers) and feeds them to four successive MFMAs.
#include "lora.h"

namespace clipfs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 zero4() {
  f32x4 z;
  z[0] = z[1] = z[2] = z[3] = 0.f;
  return z;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// fp16 storage mode: the incoming gradient is read from its f16 image (the dgrad GEMM's A operand): half the bytes
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 ld4(const _Float16* p) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(p);
  f32x4 v;
  v[0] = (float)h[0];
  v[1] = (float)h[1];
  v[2] = (float)h[2];
  v[3] = (float)h[3];
  return v;
}

// Sum the four waves' partial accumulators (the waves of a block split the reduction axis) through LDS; wave 0 gets
// the total.  red: [4 waves][NACC][64 lanes] f32x4.
template <int NACC>
__device__ __forceinline__ void block_sum4(f32x4 (&acc)[NACC], f32x4* red, int wave, int lane) {
  if (wave != 0) {
#pragma unroll
    for (int s = 0; s < NACC; ++s) red[((wave - 1) * NACC + s) * 64 + lane] = acc[s];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int s = 0; s < NACC; ++s) acc[s] += red[(w * NACC + s) * 64 + lane];
  }
}

// t = drop(x) A^T.  One block per 16 rows; its 4 waves take a quarter of the columns each (rows / 16 waves alone
// would leave ~2 waves per SIMD).  G = ceil(r / 16) rank groups of 16 output columns: every float4 of x (and its one
// Philox call) feeds all G groups, so x is read once whatever the rank.
template <int NSEG, int G>
__global__ __launch_bounds__(256) void lora_down_mfma_kernel(const float* __restrict__ x, const float* __restrict__ A,
                                                             float* __restrict__ t, int rows, int width, int r,
                                                             unsigned seg_mask, float p, uint64_t seed,
                                                             uint32_t stream_base, uint32_t drow0,
                                                             uint16_t* __restrict__ keep_bits) {
  __shared__ f32x4 red[3 * NSEG * G * 64];
  const int lane = threadIdx.x & 63, li = lane & 15, kg = lane >> 4;
  const int wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * 16;
  const int m = min(row0 + li, rows - 1);
  const bool drop = p > 0.f && seed != 0;
  const uint32_t thr = dropout_threshold(p);
  const float inv_keep = 1.f / (1.f - p);
  const float* xr = x + (size_t)m * width + 4 * kg;
  const float* ar[G];  // row of A (segment 0) this lane feeds in rank group g
#pragma unroll
  for (int g = 0; g < G; ++g) ar[g] = A + (size_t)min(16 * g + li, r - 1) * width + 4 * kg;
  f32x4 acc[NSEG * G];  // [s][g]
#pragma unroll
  for (int s = 0; s < NSEG * G; ++s) acc[s] = zero4();
  const int cw = width >> 2;  // columns per wave (width % 64 == 0)
  const int cend = (wave + 1) * cw;
  for (int c0 = wave * cw; c0 < cend; c0 += 64) {  // 4 steps of 16 columns, loads first
    f32x4 xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int cu = c0 + 16 * u;
      xv[u] = ld4(xr + min(cu, cend - 16));
      if (cu >= cend) xv[u] = zero4();
    }
    uint32_t kb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
      if (!((seg_mask >> s) & 1u)) continue;
      f32x4 wv[G][4];
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int u = 0; u < 4; ++u) wv[g][u] = ld4(ar[g] + (size_t)s * r * width + min(c0 + 16 * u, cend - 16));
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f32x4 xs = xv[u];
        if (drop) {
          const float4 mk = dropout_scale4(seed, stream_base + s, drow0 + (uint32_t)m, (uint32_t)(((c0 + 16 * u) >> 2) + kg), thr, inv_keep);
          xs[0] *= mk.x;
          xs[1] *= mk.y;
          xs[2] *= mk.z;
          xs[3] *= mk.w;
          kb[u] |= keep_bits4(mk) << (4 * s);
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[s * G + g] = mfma16(xs[e], wv[g][u][e], acc[s * G + g]);
      }
    }
    if (keep_bits && drop && row0 + li < rows) {  // the masks of this pass, for the backward (4 bits per segment and float4)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c0 + 16 * u < cend) keep_bits[(size_t)m * (width >> 2) + ((c0 + 16 * u) >> 2) + kg] = (uint16_t)kb[u];
    }
  }
  block_sum4<NSEG * G>(acc, red, wave, lane);
  if (wave == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int j = 16 * g + li;
      if (j >= r) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int mo = row0 + 4 * kg + v;
        if (mo < rows) {
#pragma unroll
          for (int s = 0; s < NSEG; ++s) t[(size_t)mo * (NSEG * r) + s * r + j] = ((seg_mask >> s) & 1u) ? acc[s * G + g][v] : 0.f;
        }
      }
    }
  }
}

// dt = scale * dy_seg B_seg.  One block (index bx) per 16 rows; each float4 of dy feeds all G rank groups.
template <int NSEG, int G, typename TY>
__device__ __forceinline__ void lora_dt_mfma_body(const TY* __restrict__ dy, const float* __restrict__ B,
                                                  float* __restrict__ dt, int rows, int segw, int r, unsigned seg_mask,
                                                  float scale, int bx, f32x4* red) {
  const int lane = threadIdx.x & 63, li = lane & 15, kg = lane >> 4;
  const int wave = threadIdx.x >> 6;
  const int row0 = bx * 16;
  const int m = min(row0 + li, rows - 1);
  const int cw = segw >> 2;
  const TY* dr = dy + (size_t)m * NSEG * segw + 4 * kg;
  f32x4 acc[NSEG * G];  // [s][g]
#pragma unroll
  for (int s = 0; s < NSEG * G; ++s) acc[s] = zero4();
#pragma unroll
  for (int s = 0; s < NSEG; ++s) {
    if (!((seg_mask >> s) & 1u)) continue;
    const float* bs[G];  // column of B this lane feeds in rank group g
#pragma unroll
    for (int g = 0; g < G; ++g) bs[g] = B + ((size_t)s * segw + 4 * kg) * r + min(16 * g + li, r - 1);
    const int cend = (wave + 1) * cw;
    for (int c0 = wave * cw; c0 < cend; c0 += 64) {
      f32x4 gv[4];
      float bv[4][G][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int cu = min(c0 + 16 * u, cend - 16);
        gv[u] = ld4(dr + s * segw + cu);
        if (c0 + 16 * u >= cend) gv[u] = zero4();
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float* bp = bs[g] + (size_t)cu * r;
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[u][g][e] = bp[e * r];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int g = 0; g < G; ++g) acc[s * G + g] = mfma16(gv[u][e], bv[u][g][e], acc[s * G + g]);
    }
  }
  block_sum4<NSEG * G>(acc, red, wave, lane);
  if (wave == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int j = 16 * g + li;
      if (j >= r) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int mo = row0 + 4 * kg + v;
        if (mo < rows) {
#pragma unroll
          for (int s = 0; s < NSEG; ++s) dt[(size_t)mo * (NSEG * r) + s * r + j] = scale * acc[s * G + g][v];
        }
      }
    }
  }
}

// dB partials: part[slice][n][j] = sum_{m in slice} dy[m, n] t[m, seg(n) r + j].  One wave per (64 columns, slice);
// lane i owns columns n0 + 4 i + e of MFMA tile e; each float4 of dy feeds all G rank groups.
template <int G, typename TY>
__device__ __forceinline__ void lora_db_mfma_body(const TY* __restrict__ dy, const float* __restrict__ t,
                                                  float* __restrict__ part, int rows, int cols, int segw, int nseg, int r,
                                                  int rows_per_slice, int bx, int by) {
  const int lane = threadIdx.x & 63, li = lane & 15, kg = lane >> 4;
  const int n0 = (bx * 4 + (threadIdx.x >> 6)) * 64;
  if (n0 >= cols) return;
  const int slice = by;
  const int m0 = slice * rows_per_slice, m1 = min(rows, m0 + rows_per_slice);
  const int s = n0 / segw;
  const int tw = nseg * r;
  const TY* dp = dy + n0 + 4 * li;
  const float* tp[G];  // rank column of t this lane feeds in group g
#pragma unroll
  for (int g = 0; g < G; ++g) tp[g] = t + s * r + min(16 * g + li, r - 1);
  f32x4 acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[g][e] = zero4();

  for (int mb = m0; mb < m1; mb += 16) {  // 4 steps of 4 rows, loads first
    f32x4 gv[4];
    float tv[4][G];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = mb + 4 * u + kg;
      const bool ok = m < m1;
      const int mc = ok ? m : m1 - 1;
      gv[u] = ld4(dp + (size_t)mc * cols);
#pragma unroll
      for (int g = 0; g < G; ++g) tv[u][g] = tp[g][(size_t)mc * tw];
      if (!ok) {
        gv[u] = zero4();
#pragma unroll
        for (int g = 0; g < G; ++g) tv[u][g] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g][e] = mfma16(gv[u][e], tv[u][g], acc[g][e]);
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int j = 16 * g + li;
    if (j >= r) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int v = 0; v < 4; ++v) part[((size_t)slice * cols + n0 + 4 * (4 * kg + v) + e) * r + j] = acc[g][e][v];
  }
}

// dA partials: part[slice][s r + j][k] = sum_{m in slice} dt[m, s r + j] drop_s(x)[m, k].  One wave per (64 columns,
// slice); lane i owns columns k0 + 4 i + e of MFMA tile e (so one Philox call covers the lane's float4 of x, and that
// float4 feeds all G rank groups).
// XACT: x holds a pre-activation u and the adapter's input is QuickGELU(u), applied as the float4 is loaded.
template <int NSEG, int G, bool XACT = false>
__device__ __forceinline__ void lora_da_mfma_body(const float* __restrict__ x, const float* __restrict__ dt,
                                                  float* __restrict__ part, int rows, int width, int r, unsigned seg_mask,
                                                  float p, uint64_t seed, uint32_t stream_base, uint32_t drow0,
                                                  int rows_per_slice, int bx, int by,
                                                  const uint16_t* __restrict__ keep_bits) {
  const int lane = threadIdx.x & 63, li = lane & 15, kg = lane >> 4;
  const int k0 = (bx * 4 + (threadIdx.x >> 6)) * 64;
  if (k0 >= width) return;
  const int slice = by;
  const int m0 = slice * rows_per_slice, m1 = min(rows, m0 + rows_per_slice);
  const bool drop = p > 0.f && seed != 0;
  const uint32_t thr = dropout_threshold(p);
  const float inv_keep = 1.f / (1.f - p);
  const int tw = NSEG * r;
  const float* xp = x + k0 + 4 * li;
  const float* dp[G];  // rank column of dt this lane feeds in group g
#pragma unroll
  for (int g = 0; g < G; ++g) dp[g] = dt + min(16 * g + li, r - 1);
  const uint32_t c4 = (uint32_t)((k0 >> 2) + li);
  f32x4 acc[NSEG][G][4];
#pragma unroll
  for (int s = 0; s < NSEG; ++s)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[s][g][e] = zero4();
  for (int mb = m0; mb < m1; mb += 8) {  // 2 steps of 4 rows, loads first
    f32x4 xv[2];
    float gv[2][NSEG][G];
    int mcs[2];
    uint32_t kbu[2] = {0u, 0u};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = mb + 4 * u + kg;
      const bool ok = m < m1;
      mcs[u] = ok ? m : m1 - 1;
      xv[u] = ld4(xp + (size_t)mcs[u] * width);
      if (keep_bits) kbu[u] = keep_bits[(size_t)mcs[u] * (width >> 2) + c4];
      if (XACT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[u][e] = quick_gelu(xv[u][e]);
      }
      if (!ok) xv[u] = zero4();
#pragma unroll
      for (int s = 0; s < NSEG; ++s)
#pragma unroll
        for (int g = 0; g < G; ++g) gv[u][s][g] = dp[g][(size_t)mcs[u] * tw + s * r];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int s = 0; s < NSEG; ++s) {
        if (!((seg_mask >> s) & 1u)) continue;
        f32x4 xs = xv[u];
        if (drop) {
          const float4 mk = keep_bits ? keep_scale4(kbu[u] >> (4 * s), inv_keep)
                                      : dropout_scale4(seed, stream_base + s, drow0 + (uint32_t)mcs[u], c4, thr, inv_keep);
          xs[0] *= mk.x;
          xs[1] *= mk.y;
          xs[2] *= mk.z;
          xs[3] *= mk.w;
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[s][g][e] = mfma16(gv[u][s][g], xs[e], acc[s][g][e]);
      }
  }
  // result tile e: D[i = rank index 16 g + 4 kg + v][j = li] <-> column k0 + 4 li + e: one float4 per (s, g, v)
#pragma unroll
  for (int s = 0; s < NSEG; ++s)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int j = 16 * g + 4 * kg + v;
        if (j < r) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = acc[s][g][e][v];
          *reinterpret_cast<f32x4*>(part + ((size_t)slice * tw + s * r + j) * width + k0 + 4 * li) = o;
        }
      }
}

// dx[m, k] += sum_s dropscale_s(m, k) sum_j dt[m, s r + j] A[s r + j, k].  One block per 16 rows (its 4 waves take a
// quarter of the columns each); per 16-column tile
// the result D[i <-> column k0 + i][j <-> row] gives a lane 4 consecutive columns of one row: a float4 of dx.
// RQ = ceil(r / 4) MFMA K-steps for r <= 16 (one rank group), 4 G above (ranks past r enter as zeros).  The lane's
// dt values stay in registers for the whole row.  Rank group 0's A values are loaded first, as at r <= 16; groups
// 1 ... G-1 are streamed (4 K-steps at a time) from one base per segment, so that neither the A values nor their
// addresses held at once grow with the rank.
template <int NSEG, int RQ>
__device__ __forceinline__ void lora_dx_mfma_body(const float* __restrict__ dt, const float* __restrict__ A,
                                                  float* __restrict__ dx, int rows, int width, int r, unsigned seg_mask,
                                                  float p, uint64_t seed, uint32_t stream_base, uint32_t drow0, int bx,
                                                  const uint16_t* __restrict__ keep_bits) {
  constexpr int QG = RQ < 4 ? RQ : 4;  // K-steps per rank group
  constexpr int G = (RQ + 3) / 4;
  const int lane = threadIdx.x & 63, li = lane & 15, kg = lane >> 4;
  const int wave = threadIdx.x >> 6;
  const int row0 = bx * 16;
  const int m = row0 + li;
  const int mc = min(m, rows - 1);
  const int cw = width >> 2;
  const bool drop = p > 0.f && seed != 0;
  const uint32_t thr = dropout_threshold(p);
  const float inv_keep = 1.f / (1.f - p);
  float dtv[NSEG][RQ];  // B operand: k = rank index 4 q + kg, j = row li
  const float* ap[NSEG][QG];  // rank group 0's rows of A
#pragma unroll
  for (int q = 0; q < RQ; ++q) {
    const int j = 4 * q + kg;
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
      dtv[s][q] = dt[(size_t)mc * (NSEG * r) + s * r + min(j, r - 1)] * (j < r ? 1.f : 0.f);
      if (q < QG) ap[s][q] = A + (size_t)(s * r + min(j, r - 1)) * width + li;
    }
  }
  float* xr = dx + (size_t)mc * width + 4 * kg;
  for (int k0 = wave * cw; k0 < (wave + 1) * cw; k0 += 32) {  // two 16-column tiles, loads first (cw % 32 == 0)
    f32x4 tot[2];
    float av[2][NSEG][QG];
    uint32_t kbu[2] = {0u, 0u};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      tot[u] = ld4(xr + k0 + 16 * u);
      if (keep_bits) kbu[u] = keep_bits[(size_t)mc * (width >> 2) + ((k0 + 16 * u) >> 2) + kg];
#pragma unroll
      for (int s = 0; s < NSEG; ++s)
#pragma unroll
        for (int q = 0; q < QG; ++q) av[u][s][q] = ap[s][q][k0 + 16 * u];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int s = 0; s < NSEG; ++s) {
        if (!((seg_mask >> s) & 1u)) continue;
        f32x4 acc = zero4();
#pragma unroll
        for (int q = 0; q < QG; ++q) acc = mfma16(av[u][s][q], dtv[s][q], acc);
#pragma unroll
        for (int g = 1; g < G; ++g) {  // r > 16: the further rank groups, streamed
          float ag[4];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            ag[q] = A[(size_t)(s * r + min(4 * (4 * g + q) + kg, r - 1)) * width + li + k0 + 16 * u];
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = mfma16(ag[q], dtv[s][4 * g + q], acc);
        }
        if (drop) {
          const float4 mk = keep_bits ? keep_scale4(kbu[u] >> (4 * s), inv_keep)
                                      : dropout_scale4(seed, stream_base + s, drow0 + (uint32_t)mc, (uint32_t)(((k0 + 16 * u) >> 2) + kg), thr, inv_keep);
          acc[0] *= mk.x;
          acc[1] *= mk.y;
          acc[2] *= mk.z;
          acc[3] *= mk.w;
        }
        tot[u] += acc;
      }
      if (m < rows) *reinterpret_cast<f32x4*>(xr + k0 + 16 * u) = tot[u];
    }
  }
}

// ---- the backward as three launches ---------------------------------------------------------------------------
// dB partials || dt, dA partials || dx, both slice sums: each pair is ONE launch whose leading blocks do the first
// product and whose trailing blocks do the second (the bodies above: same arithmetic, same results).  At the per-rank
// sizes of the 8-GPU step every product is a few microseconds of work behind ~10 us of launch, and the two halves of a
// pair fill each other's tail.
template <int NSEG, int G, typename TY>
__global__ __launch_bounds__(256) void lora_db_dt_mfma_kernel(const TY* __restrict__ dy, const float* __restrict__ B,
                                                              const float* __restrict__ t, float* __restrict__ dt,
                                                              float* __restrict__ part_b, int rows, int segw, int r,
                                                              unsigned seg_mask, float scale, int rows_per_slice,
                                                              int gx_b, int n_db) {
  __shared__ f32x4 red[3 * NSEG * G * 64];
  const int b = blockIdx.x;
  if (b < n_db)
    lora_db_mfma_body<G, TY>(dy, t, part_b, rows, NSEG * segw, segw, NSEG, r, rows_per_slice, b % gx_b, b / gx_b);
  else
    lora_dt_mfma_body<NSEG, G, TY>(dy, B, dt, rows, segw, r, seg_mask, scale, b - n_db, red);
}

template <int NSEG, int RQ, bool XACT = false>
__global__ __launch_bounds__(256) void lora_da_dx_mfma_kernel(const float* __restrict__ x, const float* __restrict__ dt,
                                                              const float* __restrict__ A, float* __restrict__ part_a,
                                                              float* __restrict__ dx, int rows, int width, int r,
                                                              unsigned seg_mask, float p, uint64_t seed,
                                                              uint32_t stream_base, uint32_t drow0, int rows_per_slice,
                                                              int gx_a, int n_da, const uint16_t* __restrict__ keep_bits) {
  const int b = blockIdx.x;
  if (b < n_da)
    lora_da_mfma_body<NSEG, (RQ + 3) / 4, XACT>(x, dt, part_a, rows, width, r, seg_mask, p, seed, stream_base, drow0, rows_per_slice,
                                          b % gx_a, b / gx_a, keep_bits);
  else
    lora_dx_mfma_body<NSEG, RQ>(dt, A, dx, rows, width, r, seg_mask, p, seed, stream_base, drow0, b - n_da, keep_bits);
}

// ---- host side: the plan (lora.hip) says what to launch; the switches below only select the compiled instance ------

template <int NSEG>
static int lora_down_mfma_s(const LoraCall& c, const LoraPlan& p) {
  decltype(&lora_down_mfma_kernel<NSEG, 1>) down = nullptr;
  switch (p.groups) {
    case 1: down = lora_down_mfma_kernel<NSEG, 1>; break;
    case 2: down = lora_down_mfma_kernel<NSEG, 2>; break;
    case 3: down = lora_down_mfma_kernel<NSEG, 3>; break;
    case 4: down = lora_down_mfma_kernel<NSEG, 4>; break;
  }
  CLIPFS_REQUIRE(down, "lora_down: no matrix-core instance for %d rank groups", p.groups);
  lora_launch(down, p.launch[0], c.st, c.x, c.A, c.t, c.rows, c.width, c.r, c.seg_mask, c.p, c.seed, c.stream_base, c.drow0,
                     c.keep_bits);
  return launch_status();
}

int lora_down_mfma(const LoraCall& c, const LoraPlan& p) {
  return c.nseg == 1 ? lora_down_mfma_s<1>(c, p) : lora_down_mfma_s<3>(c, p);
}

template <int NSEG, typename TY, bool XACT = false>
static int lora_bwd_mfma_s(const LoraCall& c, const LoraPlan& p) {
  decltype(&lora_db_dt_mfma_kernel<NSEG, 1, TY>) db_dt = nullptr;
  switch (p.groups) {
    case 1: db_dt = lora_db_dt_mfma_kernel<NSEG, 1, TY>; break;
    case 2: db_dt = lora_db_dt_mfma_kernel<NSEG, 2, TY>; break;
    case 3: db_dt = lora_db_dt_mfma_kernel<NSEG, 3, TY>; break;
    case 4: db_dt = lora_db_dt_mfma_kernel<NSEG, 4, TY>; break;
  }
  decltype(&lora_da_dx_mfma_kernel<NSEG, 1, XACT>) da_dx = nullptr;
  switch (p.rq) {
    case 1: da_dx = lora_da_dx_mfma_kernel<NSEG, 1, XACT>; break;
    case 2: da_dx = lora_da_dx_mfma_kernel<NSEG, 2, XACT>; break;
    case 3: da_dx = lora_da_dx_mfma_kernel<NSEG, 3, XACT>; break;
    case 4: da_dx = lora_da_dx_mfma_kernel<NSEG, 4, XACT>; break;
    case 8: da_dx = lora_da_dx_mfma_kernel<NSEG, 8, XACT>; break;
    case 12: da_dx = lora_da_dx_mfma_kernel<NSEG, 12, XACT>; break;
    case 16: da_dx = lora_da_dx_mfma_kernel<NSEG, 16, XACT>; break;
  }
  CLIPFS_REQUIRE(db_dt && da_dx, "lora_bwd: no matrix-core instance for %d rank groups, %d dA / dx K-steps", p.groups, p.rq);
  const int gx_b = (NSEG * c.segw + 255) / 256, gx_a = (c.width + 255) / 256;  // blocks per slice of the partials
  float* part_a = c.work + p.part_a_offset;
  lora_launch(db_dt, p.launch[0], c.st, static_cast<const TY*>(c.dy), c.B, c.t, c.dt, c.work, c.rows, c.segw, c.r, c.seg_mask,
                     c.scale, p.sr_b, gx_b, gx_b * p.slices_b);
  CLIPFS_CHECK(launch_status());
  if (p.launches > 1)
    lora_launch(da_dx, p.launch[1], c.st, c.x, c.dt, c.A, part_a, c.dx, c.rows, c.width, c.r, c.seg_mask, c.p, c.seed,
                       c.stream_base, c.drow0, p.sr_a, gx_a, gx_a * p.slices_a, c.keep_bits);
  CLIPFS_CHECK(launch_status());
  if (p.launches > 2)
    launch_reduce_slices2(p.launch[2], c.work, c.dB, (size_t)NSEG * c.segw * c.r, p.slices_b, c.scale, part_a, c.dA,
                          (size_t)NSEG * c.r * c.width, p.slices_a, 1.0f, c.st);
  return launch_status();
}

int lora_bwd_mfma(const LoraCall& c, const LoraPlan& p) {
  if (c.dy_f16) return c.nseg == 1 ? lora_bwd_mfma_s<1, _Float16>(c, p) : lora_bwd_mfma_s<3, _Float16>(c, p);
  if (c.x_act) return lora_bwd_mfma_s<1, float, true>(c, p);  // (nseg 1: the plan refuses x_act otherwise)
  return c.nseg == 1 ? lora_bwd_mfma_s<1, float>(c, p) : lora_bwd_mfma_s<3, float>(c, p);
}

}  // namespace clipfs
