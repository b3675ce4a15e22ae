// Optimal-transport matching of local image features against per-class prompt sets (clipfs.h "OT matching"; PLOT, Chen
// et al., ICLR 2023), fp32 in every engine precision mode.
//
//   z[b,c,m,n] = X[b,m,:] . P[c,n,:]     K = exp((z - 1) / eps)     v = 1
//   iters times:  u = mu / (K v)   v = nu / (K^T u)
//   T = diag(u) K diag(v)          logits[b,c] = scale sum_{m,n} T z
//
// The [B, C, M, N] similarity never leaves the chip.
//
//   logits  one workgroup per (image, chunk of classes).  The four waves form the chunk's 32 x 32 tiles of z on
//           v_mfma_f32_32x32x2_f32 straight from global memory / L2 (tile_dots_as_staged: the number the backward's
//           staged tile holds, bit for bit) into LDS.  Each wave then takes the chunk's classes one at a time: lane l
//           owns the rows l, l + 64, ... (R of them, K in R x N registers), K v is lane-local, K^T u is a per-lane sum in
//           row order followed by the wave butterfly, and v is the same number in every lane.  The last step sums T z
//           the same way.  u [B, C, M] and v [B, C, N] are outputs: the backward reads them.
//   bwd     dP and dX are one tile_grad_walk each (own rows (c, n), others (b, m), and the reverse) with
//           G = dlogits[b,c] scale u[b,c,m] v[b,c,n] exp2((z - 1) log2e / eps): T is a constant of the backward.
//
// No float atomics; every output element is written by one thread; the order of every sum depends on the shapes alone
// (a term that is skipped for a row or prompt past the end is a skipped term in every instantiation), so a (b, c) cell
// does not depend on which images and classes share the call.
#include "logits_tile.h"

#include <math.h>

namespace clipfs {
namespace {

constexpr int OT_THREADS = 256;
constexpr int OT_MAX_D = 1024, OT_MAX_M = 256, OT_MAX_N = 32;
constexpr int OT_MAX_B = 1 << 20, OT_MAX_C = 1 << 20, OT_MAX_ROWS = 1 << 24, OT_MAX_CELLS = 1 << 28;
constexpr float OT_MIN_EPS = 0.05f, OT_MAX_EPS = 10.f;
constexpr int OT_MAX_ITERS = 1000;
constexpr int OT_IDX_WORDS = 128;  // the walk's (image, row) / (class, prompt) split of 32 own and 32 other rows

__device__ __forceinline__ float ot_kernel(float z, float il2) { return __builtin_amdgcn_exp2f((z - 1.f) * il2); }

// ------------------------------------------------------------------------------------------------- logits
// LDS: zs [32 ceil(M / 32)][zst], zst = 32 (column tiles of a chunk) + 1.  R: rows per lane (ceil(M / 64) rounded up to
// 1, 2 or 4); NB: N rounded up to 4, 8, 16 or 32.
template <int R, int NB>
__global__ __launch_bounds__(OT_THREADS) void ot_logits_kernel(const float* __restrict__ X, const float* __restrict__ P,
                                                               const float* __restrict__ mu, const float* __restrict__ nu,
                                                               float* __restrict__ logits, float* __restrict__ uo,
                                                               float* __restrict__ vo, int M, int C, int N, int d, int ldl,
                                                               int cchunk, int nchunks, int zst, float il2, int iters,
                                                               float scale) {
  extern __shared__ __attribute__((aligned(16))) float ot_zs[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int b = blockIdx.x / nchunks, ch = blockIdx.x - b * nchunks;
  const int c0 = ch * cchunk, c1 = min(C, c0 + cchunk);
  const int col0 = c0 * N, ncol = (c1 - c0) * N, CN = C * N;
  const int RT = (M + 31) / 32, CT = (ncol + 31) / 32;
  const float* Xb = X + (size_t)b * M * d;
  for (int t = w; t < RT * CT; t += OT_THREADS / 64) {
    const int rt = t / CT, ct = t - rt * CT;
    const f32x16 a = tile_dots_as_staged(Xb, 32 * rt, M, P, col0 + 32 * ct, CN, d, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) ot_zs[(32 * rt + tile_row(r, h)) * zst + 32 * ct + li] = a[r];
  }
  __syncthreads();
  const float um = 1.f / (float)M, un = 1.f / (float)N;
  for (int cl = w; cl < c1 - c0; cl += OT_THREADS / 64) {  // wave-uniform
    const int c = c0 + cl;
    const size_t cell = (size_t)b * C + c;
    float K[R][NB], u[R], mur[R], v[NB], nun[NB];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int m = lane + 64 * r;
      const bool live = m < M;
      mur[r] = live ? (mu ? mu[(size_t)b * M + m] : um) : 0.f;
      u[r] = 0.f;
#pragma unroll
      for (int n = 0; n < NB; ++n) K[r][n] = live && n < N ? ot_kernel(ot_zs[m * zst + cl * N + n], il2) : 0.f;
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      v[n] = 1.f;
      nun[n] = n < N ? (nu ? nu[(size_t)c * N + n] : un) : 0.f;
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float kv = 0.f;
#pragma unroll
        for (int n = 0; n < NB; ++n)
          if (n < N) kv += K[r][n] * v[n];
        u[r] = lane + 64 * r < M ? mur[r] / kv : 0.f;
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        if (n < N) {  // wave-uniform
          float s = 0.f;
#pragma unroll
          for (int r = 0; r < R; ++r) s += K[r][n] * u[r];
          v[n] = nun[n] / wave_sum(s);
        }
      }
    }
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int m = lane + 64 * r;
      if (m < M) {
#pragma unroll
        for (int n = 0; n < NB; ++n)
          if (n < N) s += ((u[r] * K[r][n]) * v[n]) * ot_zs[m * zst + cl * N + n];
        uo[cell * M + m] = u[r];
      }
    }
    s = wave_sum(s);
    if (lane == 0) logits[(size_t)b * ldl + c] = scale * s;
#pragma unroll
    for (int n = 0; n < NB; ++n)
      if (n < N && lane == n) vo[cell * N + n] = v[n];
  }
}

// ------------------------------------------------------------------------------------------------- backward
// out[x, :] (+)= sum_y G(x, y) Y[y, :]; x = (c, n) and y = (b, m) for OWN_P (dP), the reverse otherwise (dX).
template <bool OWN_P>
struct OtGrad {
  const float* dlog;
  const float* u;
  const float* v;
  int* idx;  // [0, 32) own / [64, 96) other: image or class; [32, 64) / [96, 128): row or prompt
  int C, M, N, NY, ldd;
  float il2, scale;
  __device__ __forceinline__ void tile(int y0, int tid) const {
    if (tid < 32) {
      const int y = min(y0 + tid, NY - 1), div = OWN_P ? M : N, q = y / div;
      idx[64 + tid] = q;
      idx[96 + tid] = y - q * div;
    }
  }
  __device__ __forceinline__ float g(float a, int xi, int yi, int own, int oth) const {
    const int b = OWN_P ? idx[64 + oth] : idx[own], m = OWN_P ? idx[96 + oth] : idx[32 + own];
    const int c = OWN_P ? idx[own] : idx[64 + oth], n = OWN_P ? idx[32 + own] : idx[96 + oth];
    const size_t cell = (size_t)b * C + c;
    return dlog[(size_t)b * ldd + c] * scale * u[cell * M + m] * v[cell * N + n] * ot_kernel(a, il2);
  }
};
template <bool OWN_P, bool ACCUM, int NACC>
__global__ __launch_bounds__(OT_THREADS) void ot_bwd_kernel(const float* __restrict__ Xo, const float* __restrict__ Yo,
                                                            const float* __restrict__ dlog, const float* __restrict__ u,
                                                            const float* __restrict__ v, float* __restrict__ out, int NX,
                                                            int NY, int C, int M, int N, int d, int ldd, float il2,
                                                            float scale) {
  __shared__ int idx[OT_IDX_WORDS];
  const int tid = threadIdx.x, x0 = blockIdx.x * 32;
  if (tid < 32) {
    const int x = min(x0 + tid, NX - 1), div = OWN_P ? N : M, q = x / div;
    idx[tid] = q;
    idx[32 + tid] = x - q * div;
  }
  const OtGrad<OWN_P> fn = {dlog, u, v, idx, C, M, N, NY, ldd, il2, scale};
  tile_grad_walk<ACCUM, NACC>(Xo, Yo, out, NX, NY, d, fn);
}

// ------------------------------------------------------------------------------------------------- host
typedef struct clipfs_ot_plan OtPlan;

struct OtGradPlan {
  unsigned grid_x, grid_y, block;
  int feat_chunk;
};

float ot_il2(float eps) { return (float)(1.4426950408889634 / (double)eps); }

int ot_check_shape(int B, int M, int C, int N, int d, const char* who) {
  CLIPFS_REQUIRE(d >= 4 && d <= OT_MAX_D && d % 4 == 0, "%s: d = %d must be a multiple of 4 in [4, %d]", who, d, OT_MAX_D);
  CLIPFS_REQUIRE(M >= 1 && M <= OT_MAX_M, "%s: M = %d outside [1, %d]", who, M, OT_MAX_M);
  CLIPFS_REQUIRE(N >= 1 && N <= OT_MAX_N, "%s: N = %d outside [1, %d]", who, N, OT_MAX_N);
  CLIPFS_REQUIRE(B >= 1 && B <= OT_MAX_B, "%s: B = %d outside [1, %d]", who, B, OT_MAX_B);
  CLIPFS_REQUIRE(C >= 1 && C <= OT_MAX_C, "%s: C = %d outside [1, %d]", who, C, OT_MAX_C);
  CLIPFS_REQUIRE((long long)B * M <= OT_MAX_ROWS, "%s: B M = %lld above %d", who, (long long)B * M, OT_MAX_ROWS);
  CLIPFS_REQUIRE((long long)C * N <= OT_MAX_ROWS, "%s: C N = %lld above %d", who, (long long)C * N, OT_MAX_ROWS);
  CLIPFS_REQUIRE((long long)B * C <= OT_MAX_CELLS, "%s: B C = %lld above %d", who, (long long)B * C, OT_MAX_CELLS);
  return CLIPFS_OK;
}

int ot_check_eps(float eps, float scale, const char* who) {
  CLIPFS_REQUIRE(eps >= OT_MIN_EPS && eps <= OT_MAX_EPS, "%s: eps = %g outside [%g, %g]", who, (double)eps, (double)OT_MIN_EPS,
                 (double)OT_MAX_EPS);
  CLIPFS_REQUIRE(isfinite(scale), "%s: scale = %g must be finite", who, (double)scale);
  return CLIPFS_OK;
}

struct OtSpan {
  const char* name;
  const void* p;
  size_t bytes;
  bool written, align16, optional;
};

int ot_check_spans(const OtSpan* s, int n, const char* who) {
  for (int i = 0; i < n; ++i) {
    if (!s[i].p) {
      CLIPFS_REQUIRE(s[i].optional, "%s: %s is NULL", who, s[i].name);
      continue;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(s[i].p);
    CLIPFS_REQUIRE((a & (s[i].align16 ? 15u : 3u)) == 0, "%s: %s is not %d-byte aligned", who, s[i].name, s[i].align16 ? 16 : 4);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      if (i == j || !s[i].written || !s[i].p || !s[j].p) continue;
      const uintptr_t a = reinterpret_cast<uintptr_t>(s[i].p), c = reinterpret_cast<uintptr_t>(s[j].p);
      CLIPFS_REQUIRE(!(a < c + s[j].bytes && c < a + s[i].bytes), "%s: %s overlaps %s", who, s[i].name, s[j].name);
    }
  return CLIPFS_OK;
}

size_t ot_ld_span(int rows, int ld, int cols) { return ((size_t)(rows - 1) * ld + cols) * sizeof(float); }

template <int R, int NB>
void ot_launch_logits(const OtPlan& pl, hipStream_t st, const float* X, const float* P, const float* mu, const float* nu,
                      float* logits, float* u, float* v, int M, int C, int N, int d, int ldl, float il2, int iters, float scale) {
  if (pl.fwd_lds_bytes > 64 * 1024)  // per device, so asked for on every such call
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ot_logits_kernel<R, NB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
  hipLaunchKernelGGL((ot_logits_kernel<R, NB>), dim3(pl.fwd_grid), dim3(OT_THREADS), pl.fwd_lds_bytes, st, X, P, mu, nu, logits, u, v,
                     M, C, N, d, ldl, pl.class_chunk, pl.class_chunks, pl.z_stride, il2, iters, scale);
}

template <int R, class... Args>
void ot_launch_logits_r(const OtPlan& pl, Args... args) {
  switch (pl.prompt_regs) {
    case 4: ot_launch_logits<R, 4>(pl, args...); break;
    case 8: ot_launch_logits<R, 8>(pl, args...); break;
    case 16: ot_launch_logits<R, 16>(pl, args...); break;
    default: ot_launch_logits<R, 32>(pl, args...); break;
  }
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_ot_plan(int B, int M, int C, int N, int d, struct clipfs_ot_plan* plan) {
  const char* who = "clipfs_ot_plan";
  CLIPFS_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  CLIPFS_CHECK(ot_check_shape(B, M, C, N, d, who));
  OtPlan p = {};
  p.fwd_launches = p.dp_launches = p.dx_launches = 1;
  p.threads = OT_THREADS;
  const int RT = (M + 31) / 32, rpl = (M + 63) / 64;
  p.rows_per_lane = rpl <= 2 ? rpl : 4;
  p.prompt_regs = N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : 32;
  const int cols = RT <= 3 ? 128 : 64;  // columns of z a workgroup holds: 32 RT rows of them
  p.class_chunk = cols / N > 1 ? cols / N : 1;
  if (p.class_chunk > C) p.class_chunk = C;
  p.class_chunks = (C + p.class_chunk - 1) / p.class_chunk;
  p.z_stride = 32 * ((p.class_chunk * N + 31) / 32) + 1;
  p.fwd_grid = (unsigned)((long long)B * p.class_chunks);
  p.fwd_lds_bytes = (unsigned)((size_t)32 * RT * p.z_stride * sizeof(float));
  OtGradPlan g = {};
  tile_grad_plan(g, C * N, d);
  p.dp_grid_x = g.grid_x, p.dp_grid_y = g.grid_y, p.dp_feat_chunk = g.feat_chunk;
  tile_grad_plan(g, B * M, d);
  p.dx_grid_x = g.grid_x, p.dx_grid_y = g.grid_y, p.dx_feat_chunk = g.feat_chunk;
  p.bwd_lds_bytes = tile_grad_lds_bytes(OT_IDX_WORDS);
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_ot_logits(const float* X, const float* P, const float* mu, const float* nu, float* logits, int ldl, float* u,
                                float* v, int B, int M, int C, int N, int d, float eps, int iters, float scale, void* stream) {
  const char* who = "clipfs_ot_logits";
  OtPlan pl;
  CLIPFS_CHECK(ot_check_shape(B, M, C, N, d, who));
  CLIPFS_CHECK(clipfs_ot_plan(B, M, C, N, d, &pl));
  CLIPFS_CHECK(ot_check_eps(eps, scale, who));
  CLIPFS_REQUIRE(iters >= 1 && iters <= OT_MAX_ITERS, "%s: iters = %d outside [1, %d]", who, iters, OT_MAX_ITERS);
  CLIPFS_REQUIRE(ldl >= C, "%s: ldl = %d below C = %d", who, ldl, C);
  const size_t cells = (size_t)B * C;
  const OtSpan s[] = {
      {"X", X, (size_t)B * M * d * 4, false, true, false},   {"P", P, (size_t)C * N * d * 4, false, true, false},
      {"mu", mu, (size_t)B * M * 4, false, false, true},     {"nu", nu, (size_t)C * N * 4, false, false, true},
      {"logits", logits, ot_ld_span(B, ldl, C), true, false, false},
      {"u", u, cells * M * 4, true, false, false},           {"v", v, cells * N * 4, true, false, false},
  };
  CLIPFS_CHECK(ot_check_spans(s, 7, who));
  hipStream_t st = (hipStream_t)stream;
  const float il2 = ot_il2(eps);
  switch (pl.rows_per_lane) {
    case 1: ot_launch_logits_r<1>(pl, st, X, P, mu, nu, logits, u, v, M, C, N, d, ldl, il2, iters, scale); break;
    case 2: ot_launch_logits_r<2>(pl, st, X, P, mu, nu, logits, u, v, M, C, N, d, ldl, il2, iters, scale); break;
    default: ot_launch_logits_r<4>(pl, st, X, P, mu, nu, logits, u, v, M, C, N, d, ldl, il2, iters, scale); break;
  }
  return launch_status();
}

extern "C" int clipfs_ot_bwd(const float* X, const float* P, const float* u, const float* v, const float* dlogits, int ldd, float* dP,
                             float* dX, int B, int M, int C, int N, int d, float eps, float scale, int accumulate, void* stream) {
  const char* who = "clipfs_ot_bwd";
  OtPlan pl;
  CLIPFS_CHECK(ot_check_shape(B, M, C, N, d, who));
  CLIPFS_CHECK(clipfs_ot_plan(B, M, C, N, d, &pl));
  CLIPFS_CHECK(ot_check_eps(eps, scale, who));
  CLIPFS_REQUIRE(ldd >= C, "%s: ldd = %d below C = %d", who, ldd, C);
  const size_t cells = (size_t)B * C;
  const OtSpan s[] = {
      {"X", X, (size_t)B * M * d * 4, false, true, false},
      {"P", P, (size_t)C * N * d * 4, false, true, false},
      {"u", u, cells * M * 4, false, false, false},
      {"v", v, cells * N * 4, false, false, false},
      {"dlogits", dlogits, ot_ld_span(B, ldd, C), false, false, false},
      {"dP", dP, (size_t)C * N * d * 4, true, true, false},
      {"dX", dX, (size_t)B * M * d * 4, true, true, true},
  };
  CLIPFS_CHECK(ot_check_spans(s, 7, who));
  hipStream_t st = (hipStream_t)stream;
  const float il2 = ot_il2(eps);
  OtGradPlan g = {pl.dp_grid_x, pl.dp_grid_y, OT_THREADS, pl.dp_feat_chunk};
  TILE_GRAD_LAUNCH(ot_bwd_kernel, true, accumulate != 0, g, st, P, X, dlogits, u, v, dP, C * N, B * M, C, M, N, d, ldd, il2, scale);
  if (dX) {
    g = {pl.dx_grid_x, pl.dx_grid_y, OT_THREADS, pl.dx_feat_chunk};
    TILE_GRAD_LAUNCH(ot_bwd_kernel, false, accumulate != 0, g, st, X, P, dlogits, u, v, dX, B * M, C * N, C, M, N, d, ldd, il2, scale);
  }
  return launch_status();
}
