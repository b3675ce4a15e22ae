// Symmetric CLIP pair loss (clipfs.h "clip pairs objective"): both directions of the multi-positive InfoNCE loss of
// contrastive.hip in ONE call, with the logit scale on the device (head[0] = log s, trainable), both hit counts, the
// per-row statistics of both sides and the gradients of both feature sides and of log s, fp32 in every engine mode.
//
//   s = expf(head[0])      z[i,j] = s q[i,:] . k[j,:]
//   q side: loss_i = lse_{j live} z[i,j] - mean_{j in P_i} z[i,j]      k side: the same over i with the roles swapped
//   G[i,j] = S (w_q (exp(z - lse_q[i]) - [pos] / n_i) live_k[j] + w_k (exp(z - lse_k[j]) - [pos] / m_j) live_q[i])
//   dq_i = s sum_j G[i,j] k_j      dk_j = s sum_i G[i,j] q_i      dhead = sum_ij G[i,j] z[i,j]
//
// The sum over a row of G z needs no walk of its own: sum_j (softmax_ij - [pos] / n_i) z_ij = E_softmax[z] - mean_P z, a
// row statistic.  The entry point takes no scratch: what the gradient walks need from the rows pass (lse, 1 / n) are rows
// of the OUTPUT statistics arrays, which is why the rows kernel walks ALL of the other side (chunk partials would be
// scratch).  With weight_k == 0 the key side does not exist: no statistics, no second term, contrastive.hip's call.
//
// Neither z nor G leaves the chip.  Every kernel forms 32 x 32 tiles of dot products on v_mfma_f32_32x32x2_f32
// (logits_tile.h) summed in ONE order (tile_dots_as_staged in the rows kernel, the staged tile in the gradient walks);
// a product does not depend on which operand is A and which is B, so a cell has one fp32 z in both roles and in every
// kernel (the build does not contract s * a).  No float atomics: every output element is written by one thread of one
// workgroup and the order of every sum depends on the shapes alone.
//
//   rows     ceil(R / 32) workgroups for the queries, then (both directions) ceil(N / 32) for the keys with the roles
//            swapped.  A workgroup walks ALL of the other side in tiles of 128 (one wave per 32); a lane keeps the online
//            (max, sum exp, sum exp (z - max), sum of positive z, positive count, best value, best index) of ONE own row
//            over its 16 other rows of every tile; the eight half-waves are combined in order through LDS.
//   combine  one workgroup: loss_sum, correct [2] and dhead from the statistics by a fixed-order tree.
//   grad     tile_grad_walk with G above; the statistics and groups of the own rows are put in LDS once, those of the
//            other side's tile in fn.tile.
#include "logits_tile.h"

#include <limits.h>
#include <math.h>

namespace clipfs {
namespace {

constexpr int CP_THREADS = 256;  // 4 waves
constexpr int CP_QT = 32;        // own rows per workgroup of the rows kernel
constexpr int CP_KT = 128;       // other rows per tile of its walk: 32 per wave
constexpr int CP_FIELDS = 7;     // per (own row, half-wave): max, sum exp, sum exp (z - max), positive sum, count, best value, index
constexpr int CP_STATS = 5;      // rows of a statistics array: lse, 1 / n, loss, E[z] - mean_P z, best index

__device__ __forceinline__ float cp_exp(float x) { return __builtin_amdgcn_exp2f(x * TILE_LOG2E); }

// ------------------------------------------------------------------------------------------------- rows
__global__ __launch_bounds__(CP_THREADS) void clip_pairs_rows_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const int* __restrict__ qg, const int* __restrict__ kg,
                                                                     const float* __restrict__ head, float* __restrict__ q_stats,
                                                                     float* __restrict__ k_stats, int R, int N, int d, int q_blocks) {
  __shared__ float part[CP_FIELDS][8][32];  // [field][half-wave][own row]: a half-wave's 32 lanes on 32 banks
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const bool swapped = (int)blockIdx.x >= q_blocks;  // workgroup-uniform: the key side, roles swapped
  const float* X = swapped ? k : q;
  const float* Y = swapped ? q : k;
  const int* xg = swapped ? kg : qg;
  const int* yg = swapped ? qg : kg;
  float* stats = swapped ? k_stats : q_stats;
  const int NX = swapped ? N : R, NY = swapped ? R : N;
  const int x0 = ((int)blockIdx.x - (swapped ? q_blocks : 0)) * CP_QT;
  const float s = expf(head[0]);
  const int myg = xg[min(x0 + li, NX - 1)];
  float m = -INFINITY, l = 0.f, t = 0.f, ps = 0.f, bv = -INFINITY;
  int pc = 0, bi = INT_MAX;
  for (int y0 = 0; y0 < NY; y0 += CP_KT) {
    const int yw = y0 + 32 * w;
    if (yw < NY) {  // wave-uniform
      const f32x16 a = tile_dots_as_staged(Y, yw, NY, X, x0, NX, d, lane);  // the gradient kernels' products, bit for bit
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = yw + tile_row(r, h);  // ascending in r: a strict > keeps the lowest index of a tie
        if (j < NY) {
          const int g = yg[j];
          if (g >= 0) {
            const float z = s * a[r];
            const float mn = fmaxf(m, z);
            const float sc = cp_exp(m - mn), e = cp_exp(z - mn);
            t = (m > -INFINITY ? sc * (t + l * (m - mn)) : 0.f) + e * (z - mn);
            l = l * sc + e;
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
  part[2][hw][li] = t;
  part[3][hw][li] = ps;
  part[4][hw][li] = __int_as_float(pc);
  part[5][hw][li] = bv;
  part[6][hw][li] = __int_as_float(bi);
  __syncthreads();
  if (tid < 32 && x0 + tid < NX) {
    float M = -INFINITY;
    for (int p = 0; p < 8; ++p) M = fmaxf(M, part[0][p][tid]);
    float L = 0.f, T = 0.f, PS = 0.f, BV = -INFINITY;
    int PC = 0, BI = INT_MAX;
    for (int p = 0; p < 8; ++p) {
      const float mp = part[0][p][tid];
      if (mp > -INFINITY) {
        const float sc = cp_exp(mp - M), lp = part[1][p][tid];
        L += lp * sc;
        T += sc * (part[2][p][tid] + lp * (mp - M));
      }
      PS += part[3][p][tid];
      PC += __float_as_int(part[4][p][tid]);
      const float v = part[5][p][tid];
      const int ix = __float_as_int(part[6][p][tid]);
      if (v > BV || (v == BV && ix < BI)) {
        BV = v;
        BI = ix;
      }
    }
    const bool alive = myg >= 0 && PC > 0;  // tid < 32: li == tid
    const float lse = M + logf(L);
    const float mean = PS / (float)PC;
    const size_t i = (size_t)x0 + tid, n = (size_t)NX;
    stats[i] = alive ? lse : INFINITY;  // + inf and 1 / n = 0: the row's G is exactly 0 in the gradient walks
    stats[n + i] = alive ? 1.f / (float)PC : 0.f;
    stats[2 * n + i] = alive ? lse - mean : 0.f;
    stats[3 * n + i] = alive ? (M - mean) + T / L : 0.f;
    stats[4 * n + i] = __int_as_float(myg >= 0 && BI != INT_MAX ? BI : -1);  // BI stays unset where every live z is NaN
  }
}

// ------------------------------------------------------------------------------------------------- combine
__global__ __launch_bounds__(CP_THREADS) void clip_pairs_combine_kernel(const float* __restrict__ q_stats,
                                                                        const float* __restrict__ k_stats,
                                                                        const int* __restrict__ qg, const int* __restrict__ kg,
                                                                        const float* __restrict__ state, float* __restrict__ loss_sum,
                                                                        int* __restrict__ correct, float* __restrict__ dhead,
                                                                        int dhead_accumulate, int R, int N, float weight_q,
                                                                        float weight_k) {
  __shared__ float s_sum[4][CP_THREADS];
  __shared__ int s_hit[2][CP_THREADS];
  const int tid = threadIdx.x;
  float lq = 0.f, zq = 0.f, lk = 0.f, zk = 0.f;
  int hq = 0, hk = 0;
  for (int i = tid; i < R; i += CP_THREADS) {
    lq += q_stats[2 * (size_t)R + i];
    zq += q_stats[3 * (size_t)R + i];
    const int best = __float_as_int(q_stats[4 * (size_t)R + i]);
    hq += (best >= 0 && kg[best] == qg[i]) ? 1 : 0;  // best >= 0: the row is live, and so is its best key
  }
  if (k_stats) {
    for (int j = tid; j < N; j += CP_THREADS) {
      lk += k_stats[2 * (size_t)N + j];
      zk += k_stats[3 * (size_t)N + j];
      const int best = __float_as_int(k_stats[4 * (size_t)N + j]);
      hk += (best >= 0 && qg[best] == kg[j]) ? 1 : 0;
    }
  }
  s_sum[0][tid] = lq;
  s_sum[1][tid] = zq;
  s_sum[2][tid] = lk;
  s_sum[3][tid] = zk;
  s_hit[0][tid] = hq;
  s_hit[1][tid] = hk;
  __syncthreads();
  for (int step = CP_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
#pragma unroll
      for (int f = 0; f < 4; ++f) s_sum[f][tid] += s_sum[f][tid + step];
      s_hit[0][tid] += s_hit[0][tid + step];
      s_hit[1][tid] += s_hit[1][tid + step];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float loss_q = weight_q * s_sum[0][0];
    loss_sum[0] = k_stats ? loss_q + weight_k * s_sum[2][0] : loss_q;
    if (correct) {
      correct[0] = s_hit[0][0];
      correct[1] = s_hit[1][0];
    }
    if (dhead) {
      const float S = state ? state[CLIPFS_SCALER_SCALE] : 1.f;
      const float dq0 = (weight_q * S) * s_sum[1][0];
      const float d0 = k_stats ? dq0 + (weight_k * S) * s_sum[3][0] : dq0;
      dhead[0] = dhead_accumulate ? dhead[0] + d0 : d0;
    }
  }
}

// ------------------------------------------------------------------------------------------------- gradients
// out[x, :] (+)= sum_y g(x, y) Y[y, :].  A side's term of g is  s w_side S (exp(z - lse_side[row]) - [pos] / n_side[row])
// on cells whose row of the OTHER side is live; the own side's term exists when the own side has statistics (dq: always,
// dk: both directions), the other side's likewise.  so / sy: (lse, 1 / n, group) of the 32 own rows and of the tile's 32
// other rows in LDS.
struct CpGrad {
  const float* oth_stats;
  const int* oth_g;
  float (*so)[32];
  float (*sy)[32];
  int NY;
  float s, gs_own, gs_oth;
  bool use_own, use_oth;
  __device__ __forceinline__ void tile(int y0, int tid) const {
    if (tid < 32) {
      const int yi = y0 + tid;
      const bool in = yi < NY;
      sy[0][tid] = in && use_oth ? oth_stats[yi] : INFINITY;
      sy[1][tid] = in && use_oth ? oth_stats[(size_t)NY + yi] : 0.f;
      sy[2][tid] = __int_as_float(in ? oth_g[yi] : -1);
    }
  }
  __device__ __forceinline__ float g(float a, int, int, int own, int oth) const {
    const float z = s * a;
    const int go = __float_as_int(so[2][own]), gy = __float_as_int(sy[2][oth]);
    const bool pos = go == gy;
    float t_own = 0.f, t_oth = 0.f;
    if (use_own && gy >= 0) t_own = gs_own * (cp_exp(z - so[0][own]) - (pos ? so[1][own] : 0.f));
    if (use_oth && go >= 0) t_oth = gs_oth * (cp_exp(z - sy[0][oth]) - (pos ? sy[1][oth] : 0.f));
    return use_own ? (use_oth ? t_own + t_oth : t_own) : t_oth;
  }
};
// OWN_Q: X = q (dq), the own side's term always exists; otherwise X = k (dk), the other side's does.
template <bool OWN_Q, bool ACCUM, int NACC>
__global__ __launch_bounds__(CP_THREADS) __attribute__((amdgpu_waves_per_eu(2, NACC == 4 ? 2 : 8))) void clip_pairs_grad_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ own_g, const int* __restrict__ oth_g,
    const float* __restrict__ own_stats, const float* __restrict__ oth_stats, const float* __restrict__ head,
    float* __restrict__ out, int NX, int NY, int d, float w_own, float w_oth, int both, const float* __restrict__ state) {
  __shared__ float so[3][32];
  __shared__ float sy[3][32];
  const bool use_own = OWN_Q || both != 0, use_oth = !OWN_Q || both != 0;
  const float s = expf(head[0]);
  const float S = state ? state[CLIPFS_SCALER_SCALE] : 1.f;
  const int tid = threadIdx.x;
  if (tid < 32) {
    const int xi = blockIdx.x * 32 + tid;
    const bool in = xi < NX;
    so[0][tid] = in && use_own ? own_stats[xi] : INFINITY;
    so[1][tid] = in && use_own ? own_stats[(size_t)NX + xi] : 0.f;
    so[2][tid] = __int_as_float(in ? own_g[xi] : -1);
  }  // read after the walk's first barriers
  const CpGrad fn = {oth_stats, oth_g, so, sy, NY, s, (w_own * S) * s, (w_oth * S) * s, use_own, use_oth};
  tile_grad_walk<ACCUM, NACC>(X, Y, out, NX, NY, d, fn);
}

int cp_check_shape(int R, int N, int d) {
  CLIPFS_REQUIRE(R >= 1, "clip_pairs: R = %d must be >= 1", R);
  CLIPFS_REQUIRE(N >= 1, "clip_pairs: N = %d must be >= 1", N);
  CLIPFS_REQUIRE(d >= 4 && d <= 1024 && d % 4 == 0, "clip_pairs: d = %d must be a multiple of 4 in [4, 1024]", d);
  return CLIPFS_OK;
}

bool cp_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_clip_pairs_plan(int op, int R, int N, int d, int both, struct clipfs_clip_pairs_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_clip_pairs_plan: NULL plan");
  CLIPFS_REQUIRE(op >= CLIPFS_PAIRS_OP_ROWS && op <= CLIPFS_PAIRS_OP_DK, "clipfs_clip_pairs_plan: unknown op %d", op);
  CLIPFS_REQUIRE(both == 0 || both == 1, "clipfs_clip_pairs_plan: both = %d must be 0 or 1", both);
  CLIPFS_CHECK(cp_check_shape(R, N, d));
  struct clipfs_clip_pairs_plan p = {};
  p.block = CP_THREADS;
  p.grid_y = p.grid_z = 1;
  if (op == CLIPFS_PAIRS_OP_ROWS) {
    p.grid_x = (unsigned)((R + CP_QT - 1) / CP_QT + (both ? (N + CP_QT - 1) / CP_QT : 0));
    p.lds_bytes = (unsigned)(CP_FIELDS * 8 * 32 * sizeof(float));
  } else if (op == CLIPFS_PAIRS_OP_COMBINE) {
    p.grid_x = 1;
    p.lds_bytes = (unsigned)(6 * CP_THREADS * sizeof(float));
  } else {
    tile_grad_plan(p, op == CLIPFS_PAIRS_OP_DQ ? R : N, d);
    p.lds_bytes = tile_grad_lds_bytes(6 * 32);
  }
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_clip_pairs_objective(const float* q, const float* k, const int32_t* q_group, const int32_t* k_group,
                                           const float* head, float weight_q, float weight_k, const float* scaler_state,
                                           float* q_stats, float* k_stats, float* loss_sum, int32_t* correct, float* dq,
                                           int dq_accumulate, float* dk, int dk_accumulate, float* dhead,
                                           int dhead_accumulate, int R, int N, int d, void* stream) {
  const int both = weight_k != 0.f ? 1 : 0;
  struct clipfs_clip_pairs_plan pr, pc, pq, pk;
  CLIPFS_CHECK(clipfs_clip_pairs_plan(CLIPFS_PAIRS_OP_ROWS, R, N, d, both, &pr));
  CLIPFS_CHECK(clipfs_clip_pairs_plan(CLIPFS_PAIRS_OP_COMBINE, R, N, d, both, &pc));
  CLIPFS_CHECK(clipfs_clip_pairs_plan(CLIPFS_PAIRS_OP_DQ, R, N, d, both, &pq));
  CLIPFS_CHECK(clipfs_clip_pairs_plan(CLIPFS_PAIRS_OP_DK, R, N, d, both, &pk));
  CLIPFS_REQUIRE(q && aligned16(q), "clipfs_clip_pairs_objective: q is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(k && aligned16(k), "clipfs_clip_pairs_objective: k is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(q_group, "clipfs_clip_pairs_objective: q_group is NULL");
  CLIPFS_REQUIRE(k_group, "clipfs_clip_pairs_objective: k_group is NULL");
  CLIPFS_REQUIRE(head, "clipfs_clip_pairs_objective: head is NULL");
  CLIPFS_REQUIRE(q_stats, "clipfs_clip_pairs_objective: q_stats is NULL");
  CLIPFS_REQUIRE(loss_sum, "clipfs_clip_pairs_objective: loss_sum is NULL");
  CLIPFS_REQUIRE(isfinite(weight_q), "clipfs_clip_pairs_objective: weight_q = %g must be finite", (double)weight_q);
  CLIPFS_REQUIRE(isfinite(weight_k), "clipfs_clip_pairs_objective: weight_k = %g must be finite", (double)weight_k);
  CLIPFS_REQUIRE(both || !k_stats, "clipfs_clip_pairs_objective: k_stats must be NULL when weight_k == 0");
  CLIPFS_REQUIRE(!both || k_stats, "clipfs_clip_pairs_objective: k_stats is NULL with weight_k != 0");
  CLIPFS_REQUIRE(!dq || aligned16(dq), "clipfs_clip_pairs_objective: dq is not 16-byte aligned");
  CLIPFS_REQUIRE(!dk || aligned16(dk), "clipfs_clip_pairs_objective: dk is not 16-byte aligned");
  const size_t nq = (size_t)R * d, nk = (size_t)N * d, sq = (size_t)CP_STATS * R, sk = (size_t)CP_STATS * N;
  CLIPFS_REQUIRE(!dq || (!cp_overlap(dq, nq, q, nq) && !cp_overlap(dq, nq, k, nk)), "clipfs_clip_pairs_objective: dq aliases q or k");
  CLIPFS_REQUIRE(!dk || (!cp_overlap(dk, nk, q, nq) && !cp_overlap(dk, nk, k, nk)), "clipfs_clip_pairs_objective: dk aliases q or k");
  CLIPFS_REQUIRE(!dq || !dk || !cp_overlap(dq, nq, dk, nk), "clipfs_clip_pairs_objective: dq aliases dk");
  CLIPFS_REQUIRE(!cp_overlap(head, 1, q, nq) && !cp_overlap(head, 1, k, nk), "clipfs_clip_pairs_objective: head aliases q or k");
  CLIPFS_REQUIRE((!dq || !cp_overlap(head, 1, dq, nq)) && (!dk || !cp_overlap(head, 1, dk, nk)),
                 "clipfs_clip_pairs_objective: head aliases dq or dk");
  CLIPFS_REQUIRE(!dhead || (!cp_overlap(dhead, 1, q, nq) && !cp_overlap(dhead, 1, k, nk)),
                 "clipfs_clip_pairs_objective: dhead aliases q or k");
  CLIPFS_REQUIRE(!dhead || ((!dq || !cp_overlap(dhead, 1, dq, nq)) && (!dk || !cp_overlap(dhead, 1, dk, nk))),
                 "clipfs_clip_pairs_objective: dhead aliases dq or dk");
  CLIPFS_REQUIRE(!dhead || !cp_overlap(dhead, 1, head, 1), "clipfs_clip_pairs_objective: dhead aliases head");
  CLIPFS_REQUIRE(!cp_overlap(q_stats, sq, q, nq) && !cp_overlap(q_stats, sq, k, nk) && !cp_overlap(q_stats, sq, head, 1) &&
                     (!dq || !cp_overlap(q_stats, sq, dq, nq)) && (!dk || !cp_overlap(q_stats, sq, dk, nk)) &&
                     (!dhead || !cp_overlap(q_stats, sq, dhead, 1)),
                 "clipfs_clip_pairs_objective: q_stats aliases q, k, head, dq, dk or dhead");
  CLIPFS_REQUIRE(!k_stats || (!cp_overlap(k_stats, sk, q, nq) && !cp_overlap(k_stats, sk, k, nk) && !cp_overlap(k_stats, sk, head, 1) &&
                              (!dq || !cp_overlap(k_stats, sk, dq, nq)) && (!dk || !cp_overlap(k_stats, sk, dk, nk)) &&
                              (!dhead || !cp_overlap(k_stats, sk, dhead, 1)) && !cp_overlap(k_stats, sk, q_stats, sq)),
                 "clipfs_clip_pairs_objective: k_stats aliases q, k, head, dq, dk, dhead or q_stats");
  CLIPFS_REQUIRE(!scaler_state || aligned16(scaler_state), "clipfs_clip_pairs_objective: scaler_state is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(clip_pairs_rows_kernel, dim3(pr.grid_x), dim3(pr.block), 0, st, q, k, q_group, k_group, head, q_stats,
                     k_stats, R, N, d, (R + CP_QT - 1) / CP_QT);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(clip_pairs_combine_kernel, dim3(pc.grid_x), dim3(pc.block), 0, st, q_stats, k_stats, q_group, k_group,
                     scaler_state, loss_sum, correct, dhead, dhead_accumulate, R, N, weight_q, weight_k);
  CLIPFS_CHECK(launch_status());
  if (dq) {
    TILE_GRAD_LAUNCH(clip_pairs_grad_kernel, true, dq_accumulate != 0, pq, st, q, k, q_group, k_group, q_stats, k_stats, head,
                     dq, R, N, d, weight_q, weight_k, both, scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  if (dk) {
    TILE_GRAD_LAUNCH(clip_pairs_grad_kernel, false, dk_accumulate != 0, pk, st, k, q, k_group, q_group, k_stats, q_stats, head,
                     dk, N, R, d, weight_k, weight_q, both, scaler_state);
    CLIPFS_CHECK(launch_status());
  }
  return CLIPFS_OK;
}
