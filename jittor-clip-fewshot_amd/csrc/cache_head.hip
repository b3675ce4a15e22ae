// Tip-Adapter cache head (clipfs.h "cache head"): logits, key / query gradients and the alpha / beta search over a
// class-sorted key-value cache, fp32 in every engine precision mode.
//
//   a[b,k] = f[b,:] . K[k,:]     E[b,k] = exp(-beta (1 - a[b,k]))     S[b,c] = sum of E over the keys of class c
//   logits[b,c] = base[b,c] + alpha S[b,c]
//
// The [B, NK] affinity never leaves the chip.  Every kernel forms 32 x 32 affinity tiles on v_mfma_f32_32x32x2_f32
// (logits_tile.h): in the logits and search kernels both operands are rows read straight from global memory / L2
// (tile_dots), in the backward they pass through LDS (tile_grad_walk).  No float atomics anywhere: every float output
// element is written by one thread of one workgroup, and the order of every sum depends on the shapes and `off` only.
//
//   logits  one workgroup per (32 queries, chunk of classes) walks the chunk's keys in tiles of 128 (one wave per 32
//           keys), stages E in LDS and lets one thread add each (query, class) run in ascending key order; a run that
//           straddles tiles travels in a per-query carry.
//   bwd     one workgroup per (32 own rows, 512 features): own = keys for dK, queries for df.  It walks the other side
//           in tiles of 32 ascending (tile_grad_walk) with G = alpha beta E dlogits.
//   search  one workgroup per (32 queries, beta chunk, alpha chunk) walks ALL keys; because the keys are class-sorted,
//           classes complete in ascending order, so per (query, beta, alpha) a running (best value, best class) in LDS
//           is all that is kept.  The affinity is recomputed per chunk.
#include "logits_tile.h"

#include <math.h>

namespace clipfs {
namespace {

constexpr int CH_THREADS = 256;      // 4 waves
constexpr int CH_QT = 32;            // queries (own rows) per workgroup
constexpr int CH_KT = 128;           // keys per tile of the logits / search walk: 32 per wave
constexpr int CH_SEARCH_STATE = 120 * 1024;  // bytes of LDS the search gives its (best value, best class) records
constexpr int CH_MAX_AC = 256;       // alphas per search workgroup

// the class of key k: the largest c in [0, C) with off[c] <= k (the empty classes before it share its offset)
__device__ __forceinline__ int ch_class_of(const int* __restrict__ off, int C, int k) {
  int lo = 0, hi = C - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float ch_exp(float a, float bl2) { return __builtin_amdgcn_exp2f((a - 1.f) * bl2); }

// ------------------------------------------------------------------------------------------------- logits
__global__ __launch_bounds__(CH_THREADS) void cache_logits_kernel(const float* __restrict__ f, const float* __restrict__ K,
                                                                  const int* __restrict__ off, const float* __restrict__ base,
                                                                  float* __restrict__ out, int B, int NK, int C, int d, int ldb,
                                                                  int ldo, float alpha, float beta, int cchunk) {
  __shared__ float Es[CH_KT * 32];  // [key of the tile][query]
  __shared__ float carry[2][32];    // the run that entered this tile unfinished / leaves it unfinished
  __shared__ int s_rng[2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * CH_QT;
  const int c0 = blockIdx.y * cchunk, c1 = min(C, c0 + cchunk);
  const float bl2 = beta * TILE_LOG2E;
  const int kb = min(max(off[c0], 0), NK), ke = min(max(off[c1], kb), NK);
  // empty classes: S = 0
  for (int p = tid; p < 32 * (c1 - c0); p += CH_THREADS) {
    const int q = q0 + (p & 31), c = c0 + (p >> 5);
    if (q < B && off[c + 1] <= off[c]) out[(size_t)q * ldo + c] = base ? base[(size_t)q * ldb + c] : 0.f;
  }
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += CH_KT, buf ^= 1) {
    const int k1 = min(k0 + CH_KT, ke);
    const int kw = k0 + 32 * w;
    if (kw < k1) {  // wave-uniform
      const f32x16 a = tile_dots(K, kw, NK, f, q0, B, d, 0, 64, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) Es[(32 * w + tile_row(r, h)) * 32 + li] = ch_exp(a[r], bl2);
    }
    if (tid == 0) {
      s_rng[0] = ch_class_of(off, C, k0);
      s_rng[1] = ch_class_of(off, C, k1 - 1);
    }
    __syncthreads();
    const int cf = s_rng[0], cl = min(s_rng[1], c1 - 1);
    for (int p = tid; p < 32 * (cl - cf + 1); p += CH_THREADS) {
      const int q = p & 31, c = cf + (p >> 5);
      const int rb = off[c], re = off[c + 1];
      if (re <= rb) continue;
      const int lo = max(rb, k0), hi = min(re, k1);
      float s = rb < k0 ? carry[buf][q] : 0.f;
      for (int k = lo; k < hi; ++k) s += Es[(k - k0) * 32 + q];
      if (re <= k1) {
        if (q0 + q < B) out[(size_t)(q0 + q) * ldo + c] = (base ? base[(size_t)(q0 + q) * ldb + c] : 0.f) + alpha * s;
      } else {
        carry[buf ^ 1][q] = s;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------- backward
// out[x, :] (+)= sum_y G(x, y) Y[y, :], G = alpha beta E[b,k] dlogits[b, class(k)], (b, k) = (y, x) for OWN_KEY (dK), (x, y)
// otherwise (df).
// NACC: 32-feature accumulators per wave (logits_tile.h).
template <bool OWN_KEY>
struct ChGrad {
  const int* off;
  const float* dlog;
  int* cls_s;  // [32] class of the key tile's keys
  int C, NY, ldd;
  float bl2, ab;
  __device__ __forceinline__ void tile(int y0, int tid) const {
    if (!OWN_KEY && tid < 32) cls_s[tid] = ch_class_of(off, C, min(y0 + tid, NY - 1));
  }
  __device__ __forceinline__ float g(float a, int xi, int yi, int own, int oth) const {
    const int b = OWN_KEY ? yi : xi, c = cls_s[OWN_KEY ? own : oth];
    return ab * ch_exp(a, bl2) * dlog[(size_t)b * ldd + c];
  }
};
template <bool OWN_KEY, bool ACCUM, int NACC>
__global__ __launch_bounds__(CH_THREADS) __attribute__((amdgpu_waves_per_eu(2, NACC == 4 ? 2 : 8))) void cache_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                               const int* __restrict__ off, const float* __restrict__ dlog,
                                                               float* __restrict__ out, int NX, int NY, int C, int d, int ldd,
                                                               float alpha, float beta) {
  __shared__ int cls_s[32];
  const int tid = threadIdx.x, x0 = blockIdx.x * 32;
  if (OWN_KEY && tid < 32) cls_s[tid] = ch_class_of(off, C, min(x0 + tid, NX - 1));
  const ChGrad<OWN_KEY> fn = {off, dlog, cls_s, C, NY, ldd, beta * TILE_LOG2E, alpha * beta};
  tile_grad_walk<ACCUM, NACC>(X, Y, out, NX, NY, d, fn);
}

// ------------------------------------------------------------------------------------------------- search
__global__ __launch_bounds__(CH_THREADS) void cache_search_kernel(const float* __restrict__ f, const float* __restrict__ K,
                                                                  const int* __restrict__ off, const float* __restrict__ base,
                                                                  const int64_t* __restrict__ y, const float* __restrict__ alphas,
                                                                  const float* __restrict__ betas, int* __restrict__ hits, int B,
                                                                  int NK, int C, int d, int ldb, int nA, int nB, int JB, int AC) {
  extern __shared__ __attribute__((aligned(16))) float ch_smem[];
  float* As = ch_smem;                       // [128 keys][32 queries] affinity of the tile
  float* bsk = As + CH_KT * 32;              // [128 keys][32 queries] base[q, class(k)] where key k ends its run
  float* best_v = bsk + CH_KT * 32;          // [JB][AC][32]
  int* best_c = reinterpret_cast<int*>(best_v + JB * AC * 32);
  float* carry = reinterpret_cast<float*>(best_c + JB * AC * 32);  // [JB][32] the run in progress
  float* s_al = carry + JB * 32;             // [AC]
  float* s_bl2 = s_al + AC;                  // [JB]
  int* kcls = reinterpret_cast<int*>(s_bl2 + JB);  // [128] class of the key
  int* kflag = kcls + CH_KT;                 // [128] bit 0: first key of its run, bit 1: last key of its run
  int* kemp = kflag + CH_KT;                 // [128] at a run's first key: the first of the empty classes just before it
  int* s_tail = kemp + CH_KT;                // [1] the first of the trailing empty classes

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int q = tid & 31, slot = tid >> 5;
  const int q0 = blockIdx.x * CH_QT;
  const int j0 = blockIdx.y * JB, nj = min(JB, nB - j0);
  const int i0 = blockIdx.z * AC, na = min(AC, nA - i0);
  const size_t qrow = (size_t)min(q0 + q, B - 1) * ldb;

  for (int p = tid; p < JB * AC * 32; p += CH_THREADS) {
    best_v[p] = -INFINITY;
    best_c[p] = 0;
  }
  for (int p = tid; p < JB * 32; p += CH_THREADS) carry[p] = 0.f;
  for (int p = tid; p < na; p += CH_THREADS) s_al[p] = alphas[i0 + p];
  for (int p = tid; p < nj; p += CH_THREADS) s_bl2[p] = betas[j0 + p] * TILE_LOG2E;
  if (tid == 0) {
    int e0 = C;
    while (e0 > 0 && off[e0 - 1] >= NK) --e0;
    s_tail[0] = e0;
  }
  __syncthreads();

  for (int k0 = 0; k0 < NK; k0 += CH_KT) {
    const int kn = min(CH_KT, NK - k0);
    if (32 * w < kn) {  // wave-uniform
      const f32x16 a = tile_dots(K, k0 + 32 * w, NK, f, q0, B, d, 0, 64, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) As[(32 * w + tile_row(r, h)) * 32 + li] = a[r];
    }
    if (tid < kn) {
      const int k = k0 + tid, c = ch_class_of(off, C, k);
      const int rb = off[c], fl = (rb == k ? 1 : 0) | (off[c + 1] - 1 == k ? 2 : 0);
      int e0 = c;
      if (fl & 1)
        while (e0 > 0 && off[e0 - 1] == rb) --e0;
      kcls[tid] = c;
      kflag[tid] = fl;
      kemp[tid] = e0;
    }
    __syncthreads();
    for (int p = tid; p < kn * 32; p += CH_THREADS) {
      const int kk = p >> 5;
      if (kflag[kk] & 2) bsk[p] = base ? base[(size_t)min(q0 + (p & 31), B - 1) * ldb + kcls[kk]] : 0.f;
    }
    __syncthreads();
    for (int jj = slot; jj < nj; jj += 8) {
      const float bl2 = s_bl2[jj];
      float s = carry[jj * 32 + q];
      float* bv = best_v + (size_t)jj * AC * 32 + q;
      int* bc = best_c + (size_t)jj * AC * 32 + q;
      for (int kk = 0; kk < kn; ++kk) {
        const int fl = kflag[kk];
        if (fl & 1) {
          s = 0.f;
          const int c = kcls[kk];
          for (int ce = kemp[kk]; ce < c; ++ce) {  // empty classes: base alone
            const float v = base ? base[qrow + ce] : 0.f;
            for (int i = 0; i < na; ++i)
              if (v > bv[i * 32]) {
                bv[i * 32] = v;
                bc[i * 32] = ce;
              }
          }
        }
        s += ch_exp(As[kk * 32 + q], bl2);
        if (fl & 2) {
          const float b0 = bsk[kk * 32 + q];
          const int c = kcls[kk];
          for (int i = 0; i < na; ++i) {
            const float v = b0 + s_al[i] * s;
            if (v > bv[i * 32]) {
              bv[i * 32] = v;
              bc[i * 32] = c;
            }
          }
        }
      }
      carry[jj * 32 + q] = s;
    }
    __syncthreads();
  }
  for (int jj = slot; jj < nj; jj += 8) {
    float* bv = best_v + (size_t)jj * AC * 32 + q;
    int* bc = best_c + (size_t)jj * AC * 32 + q;
    for (int ce = s_tail[0]; ce < C; ++ce) {
      const float v = base ? base[qrow + ce] : 0.f;
      for (int i = 0; i < na; ++i)
        if (v > bv[i * 32]) {
          bv[i * 32] = v;
          bc[i * 32] = ce;
        }
    }
  }
  __syncthreads();
  // hits: lanes 0..31 / 32..63 of a wave hold the 32 queries of one (beta, alpha) pair each
  const int target = q0 + q < B ? (int)y[q0 + q] : -1;
  for (int p0 = 0; p0 < nj * AC; p0 += 8) {  // uniform trip count: the ballot needs the whole wave
    const int p = p0 + slot;
    const int jj = p / AC, i = p - jj * AC;
    const bool live = p < nj * AC && i < na;
    const bool hit = live && q0 + q < B && best_c[(size_t)p * 32 + q] == target;
    const unsigned long long m = __ballot(hit);
    const int cnt = __popcll(h ? (m >> 32) : (m & 0xffffffffull));
    if (live && li == 0 && cnt > 0) atomicAdd(&hits[(size_t)(j0 + jj) * nA + i0 + i], cnt);
  }
}

// ------------------------------------------------------------------------------------------------- host
int ch_check_shape(int B, int NK, int C, int d, int nA, int nB) {
  CLIPFS_REQUIRE(B >= 1, "cache head: B = %d must be >= 1", B);
  CLIPFS_REQUIRE(NK >= 1, "cache head: NK = %d must be >= 1", NK);
  CLIPFS_REQUIRE(C >= 1, "cache head: C = %d must be >= 1", C);
  CLIPFS_REQUIRE(d >= 4 && d <= 4096 && d % 4 == 0, "cache head: d = %d must be a multiple of 4 in [4, 4096]", d);
  CLIPFS_REQUIRE(nA >= 1 && nA <= 1024, "cache head: nA = %d must be in [1, 1024]", nA);
  CLIPFS_REQUIRE(nB >= 1 && nB <= 1024, "cache head: nB = %d must be in [1, 1024]", nB);
  return CLIPFS_OK;
}

int ch_check_scalars(float alpha, float beta) {
  CLIPFS_REQUIRE(isfinite(alpha) && alpha >= 0.f, "cache head: alpha = %g must be finite and >= 0", (double)alpha);
  CLIPFS_REQUIRE(isfinite(beta) && beta >= 0.f, "cache head: beta = %g must be finite and >= 0", (double)beta);
  return CLIPFS_OK;
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_cache_plan(int op, int B, int NK, int C, int d, int nA, int nB, struct clipfs_cache_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_cache_plan: NULL plan");
  CLIPFS_REQUIRE(op >= CLIPFS_CACHE_OP_LOGITS && op <= CLIPFS_CACHE_OP_SEARCH, "clipfs_cache_plan: unknown op %d", op);
  CLIPFS_CHECK(ch_check_shape(B, NK, C, d, nA, nB));
  struct clipfs_cache_plan p = {};
  p.block = CH_THREADS;
  p.beta_chunk = p.alpha_chunk = p.class_chunk = p.feat_chunk = 0;
  p.work_floats = 0;  // no kernel of the head needs scratch: no sum is cut over workgroups
  if (op == CLIPFS_CACHE_OP_LOGITS) {
    // classes per workgroup: enough keys for a full tile on average, as many chunks as fill the machine twice
    p.grid_x = (unsigned)((B + CH_QT - 1) / CH_QT);
    const long long min_cc = ((long long)CH_KT * C + NK - 1) / NK;
    const long long want_y = (512 + p.grid_x - 1) / p.grid_x;
    long long cc = (C + want_y - 1) / want_y;
    if (cc < min_cc) cc = min_cc;
    if (cc > C) cc = C;
    if (cc < 1) cc = 1;
    p.class_chunk = (int)cc;
    p.grid_y = (unsigned)((C + cc - 1) / cc);
    p.grid_z = 1;
    p.lds_bytes = (unsigned)((CH_KT * 32 + 2 * 32 + 2) * sizeof(float));
  } else if (op == CLIPFS_CACHE_OP_BWD_DK || op == CLIPFS_CACHE_OP_BWD_DF) {
    const int own = op == CLIPFS_CACHE_OP_BWD_DK ? NK : B;
    tile_grad_plan(p, own, d);
    p.grid_z = 1;
    p.lds_bytes = tile_grad_lds_bytes(32);  // + cls_s
  } else {
    const int ac = nA < CH_MAX_AC ? nA : CH_MAX_AC;
    int jb = CH_SEARCH_STATE / (ac * 32 * 8 + 32 * 4 + 4);  // per beta: the records, its carry row, its factor
    if (jb > nB) jb = nB;
    if (jb < 1) jb = 1;
    p.alpha_chunk = ac;
    p.beta_chunk = jb;
    p.grid_x = (unsigned)((B + CH_QT - 1) / CH_QT);
    p.grid_y = (unsigned)((nB + jb - 1) / jb);
    p.grid_z = (unsigned)((nA + ac - 1) / ac);
    p.lds_bytes = (unsigned)(sizeof(float) * ((size_t)2 * CH_KT * 32 + (size_t)2 * jb * ac * 32 + (size_t)jb * 32 + ac + jb +
                                              3 * CH_KT + 4));
  }
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_cache_logits(const float* f, const float* K, const int32_t* off, const float* base, float* out, int B,
                                   int NK, int C, int d, int ldbase, int ldout, float alpha, float beta, void* stream) {
  struct clipfs_cache_plan p;
  CLIPFS_CHECK(clipfs_cache_plan(CLIPFS_CACHE_OP_LOGITS, B, NK, C, d, 1, 1, &p));
  CLIPFS_REQUIRE(f && aligned16(f), "clipfs_cache_logits: f is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(K && aligned16(K), "clipfs_cache_logits: K is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(out && aligned16(out), "clipfs_cache_logits: out is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(off, "clipfs_cache_logits: off is NULL");
  CLIPFS_REQUIRE(ldout >= C, "clipfs_cache_logits: ldout = %d below C = %d", ldout, C);
  CLIPFS_REQUIRE(!base || ldbase >= C, "clipfs_cache_logits: ldbase = %d below C = %d", ldbase, C);
  CLIPFS_REQUIRE(out != base, "clipfs_cache_logits: out aliases base");
  CLIPFS_CHECK(ch_check_scalars(alpha, beta));
  hipLaunchKernelGGL(cache_logits_kernel, dim3(p.grid_x, p.grid_y), dim3(p.block), 0, (hipStream_t)stream, f, K, off, base, out,
                     B, NK, C, d, ldbase, ldout, alpha, beta, p.class_chunk);
  return launch_status();
}

extern "C" int clipfs_cache_bwd(const float* f, const float* K, const int32_t* off, const float* dlogits, float* dK, float* df,
                                int B, int NK, int C, int d, int lddl, float alpha, float beta, void* stream) {
  struct clipfs_cache_plan pk, pf;
  CLIPFS_CHECK(clipfs_cache_plan(CLIPFS_CACHE_OP_BWD_DK, B, NK, C, d, 1, 1, &pk));
  CLIPFS_CHECK(clipfs_cache_plan(CLIPFS_CACHE_OP_BWD_DF, B, NK, C, d, 1, 1, &pf));
  CLIPFS_REQUIRE(f && aligned16(f), "clipfs_cache_bwd: f is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(K && aligned16(K), "clipfs_cache_bwd: K is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(dK && aligned16(dK), "clipfs_cache_bwd: dK is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(!df || aligned16(df), "clipfs_cache_bwd: df is not 16-byte aligned");
  CLIPFS_REQUIRE(off, "clipfs_cache_bwd: off is NULL");
  CLIPFS_REQUIRE(dlogits, "clipfs_cache_bwd: dlogits is NULL");
  CLIPFS_REQUIRE(lddl >= C, "clipfs_cache_bwd: lddl = %d below C = %d", lddl, C);
  CLIPFS_REQUIRE(dK != K && dK != f && df != f && df != K && (!df || df != dK), "clipfs_cache_bwd: dK / df alias an input");
  CLIPFS_CHECK(ch_check_scalars(alpha, beta));
  TILE_GRAD_LAUNCH_NACC(cache_bwd_kernel, true, true, pk, (hipStream_t)stream, K, f, off, dlogits, dK, NK, B, C, d, lddl, alpha,
                        beta);
  CLIPFS_CHECK(launch_status());
  if (df) {
    TILE_GRAD_LAUNCH_NACC(cache_bwd_kernel, false, false, pf, (hipStream_t)stream, f, K, off, dlogits, df, B, NK, C, d, lddl,
                          alpha, beta);
    CLIPFS_CHECK(launch_status());
  }
  return CLIPFS_OK;
}

extern "C" int clipfs_cache_search(const float* f, const float* K, const int32_t* off, const float* base, const int64_t* y,
                                   const float* alphas, const float* betas, int32_t* hits, int B, int NK, int C, int d,
                                   int ldbase, int nA, int nB, void* stream) {
  struct clipfs_cache_plan p;
  CLIPFS_CHECK(clipfs_cache_plan(CLIPFS_CACHE_OP_SEARCH, B, NK, C, d, nA, nB, &p));
  CLIPFS_REQUIRE(f && aligned16(f), "clipfs_cache_search: f is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(K && aligned16(K), "clipfs_cache_search: K is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(off && y && alphas && betas && hits, "clipfs_cache_search: off, y, alphas, betas or hits is NULL");
  CLIPFS_REQUIRE(!base || ldbase >= C, "clipfs_cache_search: ldbase = %d below C = %d", ldbase, C);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cache_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(cache_search_kernel, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(p.block), p.lds_bytes, (hipStream_t)stream, f,
                     K, off, base, y, alphas, betas, hits, B, NK, C, d, ldbase, nA, nB, p.beta_chunk, p.alpha_chunk);
  return launch_status();
}
