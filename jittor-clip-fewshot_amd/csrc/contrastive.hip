// Multi-positive InfoNCE (clipfs.h "contrastive objective"): the one-directional image<->text contrastive loss with
// group ids (UniCL / supervised-contrastive form), its hit count and both feature gradients, fp32 in every engine
// precision mode.
//
//   z[i,j] = s q[i,:] . k[j,:]      P_i = { j live : k_group[j] == q_group[i] }      n_i = |P_i|
//   loss_i = logsumexp_{j live} z[i,j] - (1/n_i) sum_{j in P_i} z[i,j]
//   G[i,j] = w S (softmax_ij - [j in P_i] / n_i)      dq_i = s sum_j G[i,j] k_j      dk_j = s sum_i G[i,j] q_i
//
// Neither z nor G leaves the chip.  Every kernel forms 32 x 32 logits tiles on v_mfma_f32_32x32x2_f32 the way
// cache_head.hip forms its affinity tiles (operands straight from global memory / L2 in the stats kernel, through LDS in
// the gradient kernels).  No float atomics: every output element is written by one thread of one workgroup and the order
// of every sum depends on the shapes alone.
//
//   stats    one workgroup per (32 queries, chunk of keys) walks the chunk in tiles of 128 keys (one wave per 32); a lane
//            keeps the running (max, sum of exponentials, sum of positive z, positive count, best value, best index) of
//            ONE query over its 16 keys of every tile; the eight half-waves are combined in order through LDS.
//   combine  one workgroup: per query the chunks in ascending order give lse_i, n_i, loss_i and the hit flag; loss_sum
//            and correct by a fixed-order tree.  A row that contributes nothing gets lse = +inf and 1/n = 0, which makes
//            its G exactly 0 in the gradient kernels.
//   grad     one workgroup per (32 own rows, chunk of features): own = queries for dq, keys for dk.  It walks the other
//            side in tiles of 32 ascending, recomputes z, forms G from lse in LDS and contracts it with the other side's
//            rows (cache_bwd_kernel's structure).
#include "common.h"

#include <limits.h>
#include <math.h>

namespace clipfs {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int CT_THREADS = 256;   // 4 waves
constexpr int CT_QT = 32;         // queries (own rows) per workgroup
constexpr int CT_KT = 128;        // keys per tile of the stats walk: 32 per wave
constexpr int CT_MAX_CHUNK = 1024;  // most keys per stats workgroup
constexpr int CT_FEAT = 512;      // most features per gradient workgroup: 4 waves x 4 accumulators x 32
constexpr int CT_PS = 33;         // row stride of the gradient kernels' logits partials (conflict-free transposed read)
constexpr int CT_FIELDS = 6;      // per (query, chunk): max, sum of exponentials, positive sum, positive count, best value, best index
constexpr float CT_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f32x16 ct_mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of the A side that register r of lane (half h) holds
__device__ __forceinline__ int ct_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// acc[A row a0 + ct_row(r, h)][B row b0 + (lane & 31)] = the dot products over d.  Rows past the end are clamped to the
// last row (their products are discarded by the caller), features >= d read as 0.
__device__ __forceinline__ f32x16 ct_dots(const float* __restrict__ A, int a0, int na, const float* __restrict__ Bm, int b0,
                                          int nb, int d, int lane) {
  const int li = lane & 31, h = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* pa = A + (size_t)min(a0 + li, na - 1) * d + 32 * h;
  const float* pb = Bm + (size_t)min(b0 + li, nb - 1) * d + 32 * h;
  for (int s = 0; s < d; s += 64) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f32x4 va, vb;
      va[0] = va[1] = va[2] = va[3] = 0.f;
      vb = va;
      if (s + 32 * h + 4 * j < d) {
        va = *reinterpret_cast<const f32x4*>(pa + s + 4 * j);
        vb = *reinterpret_cast<const f32x4*>(pb + s + 4 * j);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = ct_mfma(va[e], vb[e], acc);
    }
  }
  return acc;
}

// The gradient kernels' tile: 32 x 32 over the whole of d, the operands passing through LDS in chunks of CT_KC features.
// Wave w takes features [32 w, 32 w + 32) of every chunk, half h 16 of them.  The next chunk -- after a tile's last one,
// the first chunk of the next tile -- is fetched into registers while this one is multiplied.
constexpr int CT_KC = 128, CT_KST = CT_KC + 4;  // + 4: 16-byte rows, conflict-free ds_read_b128 over consecutive rows
struct CtStage {
  f32x4 ra[4], rb[4];
  __device__ __forceinline__ void load(const float* __restrict__ A, int a0, int na, const float* __restrict__ Bm, int b0, int nb,
                                       int d, int s, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + CT_THREADS * i, row = e >> 5, c = s + 4 * (e & 31);
      f32x4 z;
      z[0] = z[1] = z[2] = z[3] = 0.f;
      ra[i] = rb[i] = z;
      if (c < d) {
        ra[i] = *reinterpret_cast<const f32x4*>(A + (size_t)min(a0 + row, na - 1) * d + c);
        rb[i] = *reinterpret_cast<const f32x4*>(Bm + (size_t)min(b0 + row, nb - 1) * d + c);
      }
    }
  }
  __device__ __forceinline__ void store(float* sA, float* sB, int tid) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + CT_THREADS * i, at = (e >> 5) * CT_KST + 4 * (e & 31);
      *reinterpret_cast<f32x4*>(sA + at) = ra[i];
      *reinterpret_cast<f32x4*>(sB + at) = rb[i];
    }
  }
};
// `st` holds chunk 0 of this tile on entry and chunk 0 of the next tile (if any) on return.  Every thread of the
// workgroup calls it (it synchronises).
__device__ __forceinline__ f32x16 ct_dots_staged(CtStage& st, const float* __restrict__ A, int a0, int na,
                                                 const float* __restrict__ Bm, int b0, int nb, int d, int b0n, bool has_next,
                                                 float* sA, float* sB, int tid) {
  const int lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* pa = sA + li * CT_KST + 32 * w + 16 * h;
  const float* pb = sB + li * CT_KST + 32 * w + 16 * h;
  for (int s = 0; s < d; s += CT_KC) {
    __syncthreads();  // the last chunk's reads are done
    st.store(sA, sB, tid);
    __syncthreads();
    if (s + CT_KC < d) st.load(A, a0, na, Bm, b0, nb, d, s + CT_KC, tid);
    else if (has_next) st.load(A, a0, na, Bm, b0n, nb, d, 0, tid);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(pa + 4 * j);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + 4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = ct_mfma(va[e], vb[e], acc);
    }
  }
  return acc;
}

__device__ __forceinline__ float ct_exp(float x) { return __builtin_amdgcn_exp2f(x * CT_LOG2E); }

// work: CT_FIELDS planes of [chunks][R] partials, then lse [R] and 1 / n [R]
__device__ __forceinline__ float* ct_field(float* work, int f, int chunks, int R) { return work + (size_t)f * chunks * R; }

// ------------------------------------------------------------------------------------------------- stats
__global__ __launch_bounds__(CT_THREADS) void contrastive_stats_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                       const int* __restrict__ qg, const int* __restrict__ kg,
                                                                       float* __restrict__ work, int R, int N, int d, float s,
                                                                       int cchunk) {
  __shared__ float part[CT_FIELDS][8][32];  // [field][half-wave][query]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * CT_QT;
  const int c0 = blockIdx.y * cchunk, c1 = min(N, c0 + cchunk);
  const int chunks = gridDim.y;
  const int myg = qg[min(q0 + li, R - 1)];
  float m = -INFINITY, l = 0.f, ps = 0.f, bv = -INFINITY;
  int pc = 0, bi = INT_MAX;
  for (int k0 = c0; k0 < c1; k0 += CT_KT) {
    const int kw = k0 + 32 * w;
    if (kw < c1) {  // wave-uniform
      const f32x16 a = ct_dots(k, kw, N, q, q0, R, d, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = kw + ct_row(r, h);  // ascending in r: a strict > keeps the lowest index of a tie
        if (j < c1) {
          const int g = kg[j];
          if (g >= 0) {
            const float z = s * a[r];
            const float mn = fmaxf(m, z);
            l = l * ct_exp(m - mn) + ct_exp(z - mn);
            m = mn;
            if (g == myg) {
              ps += z;
              ++pc;
            }
            if (z > bv) {
              bv = z;
              bi = j;
            }
          }
        }
      }
    }
  }
  const int hw = 2 * w + h;
  part[0][hw][li] = m;
  part[1][hw][li] = l;
  part[2][hw][li] = ps;
  part[3][hw][li] = __int_as_float(pc);
  part[4][hw][li] = bv;
  part[5][hw][li] = __int_as_float(bi);
  __syncthreads();
  if (tid < 32 && q0 + tid < R) {
    float M = -INFINITY;
    for (int p = 0; p < 8; ++p) M = fmaxf(M, part[0][p][tid]);
    float L = 0.f, PS = 0.f, BV = -INFINITY;
    int PC = 0, BI = INT_MAX;
    for (int p = 0; p < 8; ++p) {
      const float mp = part[0][p][tid];
      if (mp > -INFINITY) L += part[1][p][tid] * ct_exp(mp - M);
      PS += part[2][p][tid];
      PC += __float_as_int(part[3][p][tid]);
      const float v = part[4][p][tid];
      const int ix = __float_as_int(part[5][p][tid]);
      if (v > BV || (v == BV && ix < BI)) {
        BV = v;
        BI = ix;
      }
    }
    const size_t at = (size_t)blockIdx.y * R + q0 + tid;
    ct_field(work, 0, chunks, R)[at] = M;
    ct_field(work, 1, chunks, R)[at] = L;
    ct_field(work, 2, chunks, R)[at] = PS;
    ct_field(work, 3, chunks, R)[at] = __int_as_float(PC);
    ct_field(work, 4, chunks, R)[at] = BV;
    ct_field(work, 5, chunks, R)[at] = __int_as_float(BI);
  }
}

// ------------------------------------------------------------------------------------------------- combine
__global__ __launch_bounds__(CT_THREADS) void contrastive_combine_kernel(float* __restrict__ work, const int* __restrict__ qg,
                                                                         const int* __restrict__ kg, float* __restrict__ loss_rows,
                                                                         float* __restrict__ loss_sum, int* __restrict__ correct,
                                                                         int R, int chunks, float weight) {
  __shared__ float s_loss[CT_THREADS];
  __shared__ int s_hit[CT_THREADS];
  const int tid = threadIdx.x;
  float* lse_out = work + (size_t)CT_FIELDS * chunks * R;
  float* invn_out = lse_out + R;
  float tl = 0.f;
  int th = 0;
  for (int i = tid; i < R; i += CT_THREADS) {
    float M = -INFINITY;
    for (int c = 0; c < chunks; ++c) M = fmaxf(M, ct_field(work, 0, chunks, R)[(size_t)c * R + i]);
    float L = 0.f, PS = 0.f, BV = -INFINITY;
    int PC = 0, BI = INT_MAX;
    for (int c = 0; c < chunks; ++c) {  // ascending keys: a strict > keeps the lowest index of a tie
      const size_t at = (size_t)c * R + i;
      const float mc = ct_field(work, 0, chunks, R)[at];
      if (mc > -INFINITY) L += ct_field(work, 1, chunks, R)[at] * expf(mc - M);
      PS += ct_field(work, 2, chunks, R)[at];
      PC += __float_as_int(ct_field(work, 3, chunks, R)[at]);
      const float v = ct_field(work, 4, chunks, R)[at];
      if (v > BV) {
        BV = v;
        BI = __float_as_int(ct_field(work, 5, chunks, R)[at]);
      }
    }
    const int g = qg[i];
    const bool alive = g >= 0 && PC > 0;
    const float lse = M + logf(L);
    const float loss = alive ? lse - PS / (float)PC : 0.f;
    lse_out[i] = alive ? lse : INFINITY;
    invn_out[i] = alive ? 1.f / (float)PC : 0.f;
    if (loss_rows) loss_rows[i] = loss;
    tl += loss;
    th += (alive && BI != INT_MAX && kg[BI] == g) ? 1 : 0;  // BI stays unset where every live logit is NaN
  }
  s_loss[tid] = tl;
  s_hit[tid] = th;
  __syncthreads();
  for (int step = CT_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      s_loss[tid] += s_loss[tid + step];
      s_hit[tid] += s_hit[tid + step];
    }
    __syncthreads();
  }
  if (tid == 0) {
    loss_sum[0] = weight * s_loss[0];
    if (correct) correct[0] = s_hit[0];
  }
}

// ------------------------------------------------------------------------------------------------- gradients
// out[x, :] (+)= sum_y g(x, y) Y[y, :], g = s w S (exp(z - lse_i) - [groups equal] / n_i) with (i, j) = (x, y) for OWN_Q
// (dq: X = q, Y = k), (y, x) otherwise (dk: X = k, Y = q).  NACC: 32-feature accumulators per wave, a workgroup owning
// 128 NACC features.
template <bool OWN_Q, bool ACCUM, int NACC>
__global__ __launch_bounds__(CT_THREADS) __attribute__((amdgpu_waves_per_eu(2, NACC == 4 ? 2 : 8))) void contrastive_grad_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ qg, const int* __restrict__ kg,
    const float* __restrict__ lse, const float* __restrict__ invn, float* __restrict__ out, int NX, int NY, int d, float s,
    float weight, const float* __restrict__ state) {
  __shared__ __attribute__((aligned(16))) float sX[32 * CT_KST];  // a chunk of the own rows
  __shared__ __attribute__((aligned(16))) float sY[32 * CT_KST];  //   ... of the other side's tile
  __shared__ float Ps[4][32 * CT_PS];  // per wave: [own][other] partial dot products over its features of every chunk
  __shared__ float Gs[32 * 32];        // [other][own]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * 32;
  const int fw = (blockIdx.y * 4 + w) * 32 * NACC;  // this wave's first feature
  const float gs = (weight * (state ? state[CLIPFS_SCALER_SCALE] : 1.f)) * s;
  f32x16 acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
  CtStage st;
  st.load(X, x0, NX, Y, 0, NY, d, 0, tid);
  for (int y0 = 0; y0 < NY; y0 += 32) {
    const f32x16 dots = ct_dots_staged(st, X, x0, NX, Y, y0, NY, d, y0 + 32, y0 + 32 < NY, sX, sY, tid);
    // the first accumulator's operands of the other side: in flight while G is formed
    float y0v[16];
    {
      const int ft = fw + li;
#pragma unroll
      for (int i = 0; i < 16; ++i) y0v[i] = ft < d ? Y[(size_t)min(y0 + 16 * h + i, NY - 1) * d + ft] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) Ps[w][ct_row(r, h) * CT_PS + li] = dots[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + CT_THREADS * i, own = e & 31, oth = e >> 5;
      const int at = own * CT_PS + oth;
      const float a = ((Ps[0][at] + Ps[1][at]) + Ps[2][at]) + Ps[3][at];
      const int xi = x0 + own, yi = y0 + oth;
      float g = 0.f;
      if (xi < NX && yi < NY) {
        const int qi = OWN_Q ? xi : yi, kj = OWN_Q ? yi : xi;
        const int gk = kg[kj];
        if (gk >= 0) g = gs * (ct_exp(s * a - lse[qi]) - (gk == qg[qi] ? invn[qi] : 0.f));
      }
      Gs[oth * 32 + own] = g;
    }
    __syncthreads();
    float ga[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) ga[i] = Gs[(16 * h + i) * 32 + li];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      if (fw + 32 * a < d) {  // wave-uniform
        const int ft = fw + 32 * a + li;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float yv = a == 0 ? y0v[i] : (ft < d ? Y[(size_t)min(y0 + 16 * h + i, NY - 1) * d + ft] : 0.f);
          acc[a] = ct_mfma(ga[i], yv, acc[a]);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    const int ft = fw + 32 * a + li;
    if (ft < d) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int xi = x0 + ct_row(r, h);
        if (xi < NX) {
          float* p = out + (size_t)xi * d + ft;
          *p = ACCUM ? *p + acc[a][r] : acc[a][r];
        }
      }
    }
  }
}

template <bool OWN_Q>
void ct_launch_grad(const struct clipfs_contrastive_plan& p, bool accum, hipStream_t stream, const float* X, const float* Y,
                    const int* qg, const int* kg, const float* lse, const float* invn, float* out, int NX, int NY, int d,
                    float s, float weight, const float* state) {
  const dim3 grid(p.grid_x, p.grid_y), block(p.block);
#define CT_GO(ACC, NACC)                                                                                                  \
  hipLaunchKernelGGL((contrastive_grad_kernel<OWN_Q, ACC, NACC>), grid, block, 0, stream, X, Y, qg, kg, lse, invn, out, NX, \
                     NY, d, s, weight, state)
  if (p.feat_chunk == CT_FEAT) {
    if (accum) CT_GO(true, 4); else CT_GO(false, 4);
  } else {
    if (accum) CT_GO(true, 1); else CT_GO(false, 1);
  }
#undef CT_GO
}

int ct_check_shape(int R, int N, int d) {
  CLIPFS_REQUIRE(R >= 1, "contrastive: R = %d must be >= 1", R);
  CLIPFS_REQUIRE(N >= 1, "contrastive: N = %d must be >= 1", N);
  CLIPFS_REQUIRE(d >= 4 && d <= 1024 && d % 4 == 0, "contrastive: d = %d must be a multiple of 4 in [4, 1024]", d);
  return CLIPFS_OK;
}

bool ct_overlap(const float* a, size_t na, const float* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_contrastive_plan(int op, int R, int N, int d, struct clipfs_contrastive_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_contrastive_plan: NULL plan");
  CLIPFS_REQUIRE(op >= CLIPFS_CONTRASTIVE_OP_STATS && op <= CLIPFS_CONTRASTIVE_OP_DK, "clipfs_contrastive_plan: unknown op %d",
                 op);
  CLIPFS_CHECK(ct_check_shape(R, N, d));
  struct clipfs_contrastive_plan p = {};
  p.block = CT_THREADS;
  p.grid_z = 1;
  // keys per stats workgroup: a multiple of the 128-key tile, halved from 1024 until the grid holds a workgroup per
  // compute unit (or a chunk is one tile)
  const long long qt = (R + CT_QT - 1) / CT_QT;
  int cc = CT_MAX_CHUNK;
  while (cc > CT_KT && qt * ((N + cc - 1) / cc) < 256) cc /= 2;
  const int chunks = (N + cc - 1) / cc;
  p.col_chunk = cc;
  p.chunks = chunks;
  p.work_floats = (size_t)CT_FIELDS * chunks * R + 2 * (size_t)R;
  if (op == CLIPFS_CONTRASTIVE_OP_STATS) {
    p.grid_x = (unsigned)qt;
    p.grid_y = (unsigned)chunks;
    p.lds_bytes = (unsigned)(CT_FIELDS * 8 * 32 * sizeof(float));
  } else if (op == CLIPFS_CONTRASTIVE_OP_COMBINE) {
    p.grid_x = p.grid_y = 1;
    p.lds_bytes = (unsigned)(2 * CT_THREADS * sizeof(float));
  } else {
    const int own = op == CLIPFS_CONTRASTIVE_OP_DQ ? R : N;
    p.grid_x = (unsigned)((own + 31) / 32);
    // 512 features per workgroup where that gives every compute unit one; else 128: four times the workgroups
    p.feat_chunk = (long long)p.grid_x * ((d + CT_FEAT - 1) / CT_FEAT) >= 256 ? CT_FEAT : CT_FEAT / 4;
    p.grid_y = (unsigned)((d + p.feat_chunk - 1) / p.feat_chunk);
    p.lds_bytes = (unsigned)((2 * 32 * CT_KST + 4 * 32 * CT_PS + 32 * 32) * sizeof(float));
  }
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_contrastive_objective(const float* q, const float* k, const int32_t* q_group, const int32_t* k_group,
                                            float logit_scale, float weight, const float* scaler_state, float* loss_rows,
                                            float* loss_sum, int32_t* correct, float* dq, int dq_accumulate, float* dk,
                                            int dk_accumulate, float* work, int R, int N, int d, void* stream) {
  struct clipfs_contrastive_plan ps, pc, pq, pk;
  CLIPFS_CHECK(clipfs_contrastive_plan(CLIPFS_CONTRASTIVE_OP_STATS, R, N, d, &ps));
  CLIPFS_CHECK(clipfs_contrastive_plan(CLIPFS_CONTRASTIVE_OP_COMBINE, R, N, d, &pc));
  CLIPFS_CHECK(clipfs_contrastive_plan(CLIPFS_CONTRASTIVE_OP_DQ, R, N, d, &pq));
  CLIPFS_CHECK(clipfs_contrastive_plan(CLIPFS_CONTRASTIVE_OP_DK, R, N, d, &pk));
  CLIPFS_REQUIRE(q && aligned16(q), "clipfs_contrastive_objective: q is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(k && aligned16(k), "clipfs_contrastive_objective: k is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(q_group, "clipfs_contrastive_objective: q_group is NULL");
  CLIPFS_REQUIRE(k_group, "clipfs_contrastive_objective: k_group is NULL");
  CLIPFS_REQUIRE(loss_sum, "clipfs_contrastive_objective: loss_sum is NULL");
  CLIPFS_REQUIRE(work, "clipfs_contrastive_objective: work is NULL");
  CLIPFS_REQUIRE(!dq || aligned16(dq), "clipfs_contrastive_objective: dq is not 16-byte aligned");
  CLIPFS_REQUIRE(!dk || aligned16(dk), "clipfs_contrastive_objective: dk is not 16-byte aligned");
  const size_t nq = (size_t)R * d, nk = (size_t)N * d;
  CLIPFS_REQUIRE(!dq || (!ct_overlap(dq, nq, q, nq) && !ct_overlap(dq, nq, k, nk)), "clipfs_contrastive_objective: dq aliases q or k");
  CLIPFS_REQUIRE(!dk || (!ct_overlap(dk, nk, q, nq) && !ct_overlap(dk, nk, k, nk)), "clipfs_contrastive_objective: dk aliases q or k");
  CLIPFS_REQUIRE(!dq || !dk || !ct_overlap(dq, nq, dk, nk), "clipfs_contrastive_objective: dq aliases dk");
  CLIPFS_REQUIRE(isfinite(logit_scale), "clipfs_contrastive_objective: logit_scale = %g must be finite", (double)logit_scale);
  CLIPFS_REQUIRE(isfinite(weight), "clipfs_contrastive_objective: weight = %g must be finite", (double)weight);
  CLIPFS_REQUIRE(!scaler_state || aligned16(scaler_state), "clipfs_contrastive_objective: scaler_state is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(contrastive_stats_kernel, dim3(ps.grid_x, ps.grid_y), dim3(ps.block), 0, st, q, k, q_group, k_group, work,
                     R, N, d, logit_scale, ps.col_chunk);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(contrastive_combine_kernel, dim3(pc.grid_x), dim3(pc.block), 0, st, work, q_group, k_group, loss_rows,
                     loss_sum, correct, R, ps.chunks, weight);
  CLIPFS_CHECK(launch_status());
  const float* lse = work + (size_t)CT_FIELDS * ps.chunks * R;
  const float* invn = lse + R;
  if (dq) {
    ct_launch_grad<true>(pq, dq_accumulate != 0, st, q, k, q_group, k_group, lse, invn, dq, R, N, d, logit_scale, weight,
                         scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  if (dk) {
    ct_launch_grad<false>(pk, dk_accumulate != 0, st, k, q, q_group, k_group, lse, invn, dk, N, R, d, logit_scale, weight,
                          scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  return CLIPFS_OK;
}
