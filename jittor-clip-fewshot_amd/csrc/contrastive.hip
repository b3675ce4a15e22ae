// Multi-positive InfoNCE (clipfs.h "contrastive objective"): the one-directional image<->text contrastive loss with
// group ids (UniCL / supervised-contrastive form), its hit count and both feature gradients, fp32 in every engine
// precision mode.
//
//   z[i,j] = s q[i,:] . k[j,:]      P_i = { j live : k_group[j] == q_group[i] }      n_i = |P_i|
//   loss_i = logsumexp_{j live} z[i,j] - (1/n_i) sum_{j in P_i} z[i,j]
//   G[i,j] = w S (softmax_ij - [j in P_i] / n_i)      dq_i = s sum_j G[i,j] k_j      dk_j = s sum_i G[i,j] q_i
//
// Neither z nor G leaves the chip.  Every kernel forms 32 x 32 logits tiles on v_mfma_f32_32x32x2_f32 (logits_tile.h:
// operands straight from global memory / L2 in the stats kernel, through LDS in the gradient kernels, summed in ONE
// order, so that the z behind lse and the z of the gradient are the same fp32 number; the build does not contract s * a).
// No float atomics: every output element is written by one thread of one workgroup and the order of every sum depends on
// the shapes alone.
//
//   stats    one workgroup per (32 queries, chunk of keys) walks the chunk in tiles of 128 keys (one wave per 32); a lane
//            keeps the running (max, sum of exponentials, sum of positive z, positive count, best value, best index) of
//            ONE query over its 16 keys of every tile; the eight half-waves are combined in order through LDS.
//   combine  one workgroup: per query the chunks in ascending order give lse_i, n_i, loss_i and the hit flag; loss_sum
//            and correct by a fixed-order tree.  A row that contributes nothing gets lse = +inf and 1/n = 0, which makes
//            its G exactly 0 in the gradient kernels.
//   grad     one workgroup per (32 own rows, chunk of features): own = queries for dq, keys for dk.  It walks the other
//            side in tiles of 32 ascending, recomputes z, forms G from lse in LDS and contracts it with the other side's
//            rows (tile_grad_walk).
#include "logits_tile.h"

#include <limits.h>
#include <math.h>

namespace clipfs {
namespace {

constexpr int CT_THREADS = 256;   // 4 waves
constexpr int CT_QT = 32;         // queries (own rows) per workgroup
constexpr int CT_KT = 128;        // keys per tile of the stats walk: 32 per wave
constexpr int CT_MAX_CHUNK = 1024;  // most keys per stats workgroup
constexpr int CT_FIELDS = 6;      // per (query, chunk): max, sum of exponentials, positive sum, positive count, best value, best index

__device__ __forceinline__ float ct_exp(float x) { return __builtin_amdgcn_exp2f(x * TILE_LOG2E); }

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
      const f32x16 a = tile_dots_as_staged(k, kw, N, q, q0, R, d, lane);  // the gradient kernels' z, bit for bit
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = kw + tile_row(r, h);  // ascending in r: a strict > keeps the lowest index of a tie
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
// (dq: X = q, Y = k), (y, x) otherwise (dk: X = k, Y = q).  NACC: 32-feature accumulators per wave (logits_tile.h).
template <bool OWN_Q>
struct CtGrad {
  const int *qg, *kg;
  const float *lse, *invn;
  float s, gs;
  __device__ __forceinline__ void tile(int, int) const {}
  __device__ __forceinline__ float g(float a, int xi, int yi, int, int) const {
    const int qi = OWN_Q ? xi : yi, kj = OWN_Q ? yi : xi;
    const int gk = kg[kj];
    return gk >= 0 ? gs * (ct_exp(s * a - lse[qi]) - (gk == qg[qi] ? invn[qi] : 0.f)) : 0.f;
  }
};
template <bool OWN_Q, bool ACCUM, int NACC>
__global__ __launch_bounds__(CT_THREADS) __attribute__((amdgpu_waves_per_eu(2, NACC == 4 ? 2 : 8))) void contrastive_grad_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ qg, const int* __restrict__ kg,
    const float* __restrict__ lse, const float* __restrict__ invn, float* __restrict__ out, int NX, int NY, int d, float s,
    float weight, const float* __restrict__ state) {
  const CtGrad<OWN_Q> fn = {qg, kg, lse, invn, s, (weight * (state ? state[CLIPFS_SCALER_SCALE] : 1.f)) * s};
  tile_grad_walk<ACCUM, NACC>(X, Y, out, NX, NY, d, fn);
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
    tile_grad_plan(p, own, d);
    p.lds_bytes = tile_grad_lds_bytes();
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
    TILE_GRAD_LAUNCH(contrastive_grad_kernel, true, dq_accumulate != 0, pq, st, q, k, q_group, k_group, lse, invn, dq, R, N, d,
                     logit_scale, weight, scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  if (dk) {
    TILE_GRAD_LAUNCH(contrastive_grad_kernel, false, dk_accumulate != 0, pk, st, k, q, q_group, k_group, lse, invn, dk, N, R, d,
                     logit_scale, weight, scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  return CLIPFS_OK;
}
