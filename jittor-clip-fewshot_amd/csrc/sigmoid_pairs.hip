// Pairwise sigmoid (SigLIP) loss (clipfs.h "sigmoid objective"): every (query, key) cell an independent binary problem
// with the group ids as labels, a scale and a bias that live on the device (head = (log t, b)), the hit count, the row
// statistics and the gradients of both feature sides and of the head, fp32 in every engine precision mode.
//
//   z[i,j] = t q[i,:] . k[j,:] + b      live = both groups >= 0      pos = live and groups equal
//   l[i,j] = softplus(-z) if pos else softplus(z)      G[i,j] = w S (sigmoid(z) - [pos])  on live cells
//   dq_i = t sum_j G[i,j] k_j      dk_j = t sum_i G[i,j] q_i      dhead = (t sum G a, sum G)
//
// There is no row normaliser: a live query without a positive still pays its negative terms (under InfoNCE,
// contrastive.hip, such a row contributes nothing), and the gradient kernels need nothing from an earlier pass, so the
// entry point takes no scratch: the per-row results are the output row_stats, which the combine kernel reads.
//
// Neither z nor G leaves the chip.  Every kernel forms 32 x 32 tiles of dot products on v_mfma_f32_32x32x2_f32
// (logits_tile.h), summed in ONE order (tile_dots_as_staged in the rows kernel, the staged tile in the gradient
// kernels), and every kernel makes z = t * a + b from them with the same two roundings (the build does not contract),
// so a cell has one z everywhere.  No float atomics: every output element is written by one thread of one workgroup and
// the order of every sum depends on the shapes alone.
//
//   rows     one workgroup per 32 queries walks ALL keys in tiles of 128 (one wave per 32); a lane keeps the running
//            (loss, sum of sigmoid - [pos], the same times a, best value, best index) of ONE query over its 16 keys of
//            every tile, a tile's 16 terms summed first and then added to the running sums; the eight half-waves are
//            combined in order through LDS.
//   combine  one workgroup: loss_sum, correct and dhead from row_stats by a fixed-order tree.
//   grad     tile_grad_walk with this objective's G; own = queries for dq, keys for dk.
#include "logits_tile.h"

#include <limits.h>
#include <math.h>

namespace clipfs {
namespace {

constexpr int SG_THREADS = 256;  // 4 waves
constexpr int SG_QT = 32;        // queries per workgroup of the rows kernel
constexpr int SG_KT = 128;       // keys per tile of its walk: 32 per wave
constexpr int SG_FIELDS = 5;     // per (query, half-wave): loss, sum g, sum g a, best value, best index
constexpr int SG_STATS = 4;      // rows of row_stats

// log(1 + exp(x)) with the tail kept: for x << 0 the result is exp(x) (1 - exp(x) / 2 + ...), which log(1 + u) would
// round to a multiple of 2^-24
__device__ __forceinline__ float sg_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
// 1 / (1 + exp(-x)) without an overflowing exponential
__device__ __forceinline__ float sg_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.f ? 1.f : e) / (1.f + e);
}
// sigmoid(z) - [pos], the positive side as -sigmoid(-z): no cancellation where sigmoid(z) is close to 1
__device__ __forceinline__ float sg_resid(float z, bool pos) { return pos ? -sg_sigmoid(-z) : sg_sigmoid(z); }

// ------------------------------------------------------------------------------------------------- rows
__global__ __launch_bounds__(SG_THREADS) void sigmoid_rows_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const int* __restrict__ qg, const int* __restrict__ kg,
                                                                  const float* __restrict__ head, float* __restrict__ row_stats,
                                                                  int R, int N, int d) {
  __shared__ float part[SG_FIELDS][8][32];  // [field][half-wave][query]: a half-wave's 32 lanes on 32 banks
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * SG_QT;
  const float t = expf(head[0]), b = head[1];
  const int myg = qg[min(q0 + li, R - 1)];
  float ls = 0.f, sg = 0.f, sga = 0.f, bv = -INFINITY;
  int bi = INT_MAX;
  for (int k0 = 0; k0 < N; k0 += SG_KT) {
    const int kw = k0 + 32 * w;
    if (kw < N) {  // wave-uniform
      const f32x16 a = tile_dots_as_staged(k, kw, N, q, q0, R, d, lane);  // the gradient kernels' products, bit for bit
      float tl = 0.f, tg = 0.f, tga = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = kw + tile_row(r, h);  // ascending in r: a strict > keeps the lowest index of a tie
        if (j < N) {
          const int g = kg[j];
          if (g >= 0) {
            const float z = t * a[r] + b;
            const bool pos = g == myg;
            const float gg = sg_resid(z, pos);
            tl += sg_softplus(pos ? -z : z);
            tg += gg;
            tga += gg * a[r];
            if (z > bv) {
              bv = z;
              bi = j;
            }
          }
        }
      }
      ls += tl;
      sg += tg;
      sga += tga;
    }
  }
  const int hw = 2 * w + h;
  part[0][hw][li] = ls;
  part[1][hw][li] = sg;
  part[2][hw][li] = sga;
  part[3][hw][li] = bv;
  part[4][hw][li] = __int_as_float(bi);
  __syncthreads();
  if (tid < 32 && q0 + tid < R) {
    float LS = 0.f, SG = 0.f, SGA = 0.f, BV = -INFINITY;
    int BI = INT_MAX;
    for (int p = 0; p < 8; ++p) {
      LS += part[0][p][tid];
      SG += part[1][p][tid];
      SGA += part[2][p][tid];
      const float v = part[3][p][tid];
      const int ix = __float_as_int(part[4][p][tid]);
      if (v > BV || (v == BV && ix < BI)) {
        BV = v;
        BI = ix;
      }
    }
    const bool alive = myg >= 0;  // tid < 32: li == tid
    const size_t i = (size_t)q0 + tid;
    row_stats[i] = alive ? LS : 0.f;
    row_stats[(size_t)R + i] = alive ? SG : 0.f;
    row_stats[2 * (size_t)R + i] = alive ? SGA : 0.f;
    row_stats[3 * (size_t)R + i] = __int_as_float(alive && BI != INT_MAX ? BI : -1);  // BI stays unset where every live z is NaN
  }
}

// ------------------------------------------------------------------------------------------------- combine
__global__ __launch_bounds__(SG_THREADS) void sigmoid_combine_kernel(const float* __restrict__ row_stats, const int* __restrict__ qg,
                                                                     const int* __restrict__ kg, const float* __restrict__ head,
                                                                     const float* __restrict__ state, float* __restrict__ loss_sum,
                                                                     int* __restrict__ correct, float* __restrict__ dhead,
                                                                     int dhead_accumulate, int R, float weight) {
  __shared__ float s_sum[3][SG_THREADS];
  __shared__ int s_hit[SG_THREADS];
  const int tid = threadIdx.x;
  float tl = 0.f, tg = 0.f, tga = 0.f;
  int th = 0;
  for (int i = tid; i < R; i += SG_THREADS) {
    tl += row_stats[i];
    tg += row_stats[(size_t)R + i];
    tga += row_stats[2 * (size_t)R + i];
    const int best = __float_as_int(row_stats[3 * (size_t)R + i]);
    th += (best >= 0 && kg[best] == qg[i]) ? 1 : 0;  // best >= 0: the query is live; its best key is live
  }
  s_sum[0][tid] = tl;
  s_sum[1][tid] = tg;
  s_sum[2][tid] = tga;
  s_hit[tid] = th;
  __syncthreads();
  for (int step = SG_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      s_sum[0][tid] += s_sum[0][tid + step];
      s_sum[1][tid] += s_sum[1][tid + step];
      s_sum[2][tid] += s_sum[2][tid + step];
      s_hit[tid] += s_hit[tid + step];
    }
    __syncthreads();
  }
  if (tid == 0) {
    loss_sum[0] = weight * s_sum[0][0];
    if (correct) correct[0] = s_hit[0];
    if (dhead) {
      const float gs = weight * (state ? state[CLIPFS_SCALER_SCALE] : 1.f);
      const float d0 = (gs * expf(head[0])) * s_sum[2][0], d1 = gs * s_sum[1][0];
      dhead[0] = dhead_accumulate ? dhead[0] + d0 : d0;
      dhead[1] = dhead_accumulate ? dhead[1] + d1 : d1;
    }
  }
}

// ------------------------------------------------------------------------------------------------- gradients
// out[x, :] (+)= sum_y g(x, y) Y[y, :], g = t w S (sigmoid(z) - [pos]) on live cells with (i, j) = (x, y) for OWN_Q
// (dq: X = q, Y = k), (y, x) otherwise (dk: X = k, Y = q).  NACC: 32-feature accumulators per wave (logits_tile.h).
template <bool OWN_Q>
struct SgGrad {
  const int *qg, *kg;
  float t, b, gt;
  __device__ __forceinline__ void tile(int, int) const {}
  __device__ __forceinline__ float g(float a, int xi, int yi, int, int) const {
    const int gq = qg[OWN_Q ? xi : yi], gk = kg[OWN_Q ? yi : xi];
    return gq >= 0 && gk >= 0 ? gt * sg_resid(t * a + b, gq == gk) : 0.f;
  }
};
template <bool OWN_Q, bool ACCUM, int NACC>
__global__ __launch_bounds__(SG_THREADS) __attribute__((amdgpu_waves_per_eu(2, NACC == 4 ? 2 : 8))) void sigmoid_grad_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ qg, const int* __restrict__ kg,
    const float* __restrict__ head, float* __restrict__ out, int NX, int NY, int d, float weight,
    const float* __restrict__ state) {
  const float t = expf(head[0]);
  const SgGrad<OWN_Q> fn = {qg, kg, t, head[1], (weight * (state ? state[CLIPFS_SCALER_SCALE] : 1.f)) * t};
  tile_grad_walk<ACCUM, NACC>(X, Y, out, NX, NY, d, fn);
}

int sg_check_shape(int R, int N, int d) {
  CLIPFS_REQUIRE(R >= 1, "sigmoid: R = %d must be >= 1", R);
  CLIPFS_REQUIRE(N >= 1, "sigmoid: N = %d must be >= 1", N);
  CLIPFS_REQUIRE(d >= 4 && d <= 1024 && d % 4 == 0, "sigmoid: d = %d must be a multiple of 4 in [4, 1024]", d);
  return CLIPFS_OK;
}

bool sg_overlap(const float* a, size_t na, const float* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_sigmoid_plan(int op, int R, int N, int d, struct clipfs_sigmoid_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_sigmoid_plan: NULL plan");
  CLIPFS_REQUIRE(op >= CLIPFS_SIGMOID_OP_ROWS && op <= CLIPFS_SIGMOID_OP_DK, "clipfs_sigmoid_plan: unknown op %d", op);
  CLIPFS_CHECK(sg_check_shape(R, N, d));
  struct clipfs_sigmoid_plan p = {};
  p.block = SG_THREADS;
  p.grid_y = p.grid_z = 1;
  if (op == CLIPFS_SIGMOID_OP_ROWS) {
    p.grid_x = (unsigned)((R + SG_QT - 1) / SG_QT);
    p.lds_bytes = (unsigned)(SG_FIELDS * 8 * 32 * sizeof(float));
  } else if (op == CLIPFS_SIGMOID_OP_COMBINE) {
    p.grid_x = 1;
    p.lds_bytes = (unsigned)(4 * SG_THREADS * sizeof(float));
  } else {
    tile_grad_plan(p, op == CLIPFS_SIGMOID_OP_DQ ? R : N, d);
    p.lds_bytes = tile_grad_lds_bytes();
  }
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_sigmoid_objective(const float* q, const float* k, const int32_t* q_group, const int32_t* k_group,
                                        const float* head, float weight, const float* scaler_state, float* row_stats,
                                        float* loss_sum, int32_t* correct, float* dq, int dq_accumulate, float* dk,
                                        int dk_accumulate, float* dhead, int dhead_accumulate, int R, int N, int d,
                                        void* stream) {
  struct clipfs_sigmoid_plan pr, pc, pq, pk;
  CLIPFS_CHECK(clipfs_sigmoid_plan(CLIPFS_SIGMOID_OP_ROWS, R, N, d, &pr));
  CLIPFS_CHECK(clipfs_sigmoid_plan(CLIPFS_SIGMOID_OP_COMBINE, R, N, d, &pc));
  CLIPFS_CHECK(clipfs_sigmoid_plan(CLIPFS_SIGMOID_OP_DQ, R, N, d, &pq));
  CLIPFS_CHECK(clipfs_sigmoid_plan(CLIPFS_SIGMOID_OP_DK, R, N, d, &pk));
  CLIPFS_REQUIRE(q && aligned16(q), "clipfs_sigmoid_objective: q is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(k && aligned16(k), "clipfs_sigmoid_objective: k is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(q_group, "clipfs_sigmoid_objective: q_group is NULL");
  CLIPFS_REQUIRE(k_group, "clipfs_sigmoid_objective: k_group is NULL");
  CLIPFS_REQUIRE(head, "clipfs_sigmoid_objective: head is NULL");
  CLIPFS_REQUIRE(row_stats, "clipfs_sigmoid_objective: row_stats is NULL");
  CLIPFS_REQUIRE(loss_sum, "clipfs_sigmoid_objective: loss_sum is NULL");
  CLIPFS_REQUIRE(!dq || aligned16(dq), "clipfs_sigmoid_objective: dq is not 16-byte aligned");
  CLIPFS_REQUIRE(!dk || aligned16(dk), "clipfs_sigmoid_objective: dk is not 16-byte aligned");
  const size_t nq = (size_t)R * d, nk = (size_t)N * d;
  CLIPFS_REQUIRE(!dq || (!sg_overlap(dq, nq, q, nq) && !sg_overlap(dq, nq, k, nk)), "clipfs_sigmoid_objective: dq aliases q or k");
  CLIPFS_REQUIRE(!dk || (!sg_overlap(dk, nk, q, nq) && !sg_overlap(dk, nk, k, nk)), "clipfs_sigmoid_objective: dk aliases q or k");
  CLIPFS_REQUIRE(!dq || !dk || !sg_overlap(dq, nq, dk, nk), "clipfs_sigmoid_objective: dq aliases dk");
  CLIPFS_REQUIRE(!sg_overlap(head, 2, q, nq) && !sg_overlap(head, 2, k, nk), "clipfs_sigmoid_objective: head aliases q or k");
  CLIPFS_REQUIRE((!dq || !sg_overlap(head, 2, dq, nq)) && (!dk || !sg_overlap(head, 2, dk, nk)),
                 "clipfs_sigmoid_objective: head aliases dq or dk");
  CLIPFS_REQUIRE(!dhead || (!sg_overlap(dhead, 2, q, nq) && !sg_overlap(dhead, 2, k, nk)),
                 "clipfs_sigmoid_objective: dhead aliases q or k");
  CLIPFS_REQUIRE(!dhead || ((!dq || !sg_overlap(dhead, 2, dq, nq)) && (!dk || !sg_overlap(dhead, 2, dk, nk))),
                 "clipfs_sigmoid_objective: dhead aliases dq or dk");
  CLIPFS_REQUIRE(!dhead || !sg_overlap(dhead, 2, head, 2), "clipfs_sigmoid_objective: dhead aliases head");
  CLIPFS_REQUIRE(isfinite(weight), "clipfs_sigmoid_objective: weight = %g must be finite", (double)weight);
  CLIPFS_REQUIRE(!scaler_state || aligned16(scaler_state), "clipfs_sigmoid_objective: scaler_state is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sigmoid_rows_kernel, dim3(pr.grid_x), dim3(pr.block), 0, st, q, k, q_group, k_group, head, row_stats, R, N,
                     d);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(sigmoid_combine_kernel, dim3(pc.grid_x), dim3(pc.block), 0, st, row_stats, q_group, k_group, head,
                     scaler_state, loss_sum, correct, dhead, dhead_accumulate, R, weight);
  CLIPFS_CHECK(launch_status());
  if (dq) {
    TILE_GRAD_LAUNCH(sigmoid_grad_kernel, true, dq_accumulate != 0, pq, st, q, k, q_group, k_group, head, dq, R, N, d, weight,
                     scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  if (dk) {
    TILE_GRAD_LAUNCH(sigmoid_grad_kernel, false, dk_accumulate != 0, pk, st, k, q, q_group, k_group, head, dk, N, R, d, weight,
                     scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  return CLIPFS_OK;
}
