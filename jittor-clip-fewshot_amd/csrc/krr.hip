// Kernel ridge regression head (clipfs.h "KRR"; ProKeR: Bendou et al., CVPR 2025), fp32: the Tip-Adapter kernel
// k(x, s) = exp(-beta (1 - x . s)) with the closed-form ridge solution At = Et (k(S, S) + lambda I)^-1 by the Cholesky
// factor and solve of spd.hip, and the product out = base + k(X, S) At^T with a dense At.
//
//   system   clipfs_gemm_nt (S S^T into A), then the map in place: exp2((a - 1) beta log2 e), + lambda on the diagonal,
//            the identity in the pad rows and columns n .. n4.  One thread per float4.
//   targets  Et[c, j] = t [labels[j] == c] - base_S[j, c], pad columns 0; one thread per element, coalesced along j.
//   apply    one workgroup per 32 query rows and class chunk.  It walks the keys in tiles of 32: both operands staged
//            through LDS (tile_dots_staged of logits_tile.h), the waves' partials added in wave order, g formed once in
//            LDS; then wave w contracts g with the rows of At of its class tiles (tile 4 a + w of the chunk for its
//            accumulator a) on the matrix cores: a lane reads 16 contiguous key columns of one class row per tile.  NT
//            accumulators per wave stay in registers over the whole walk.
//
// No atomics; every output element is written by one thread; the order of every sum depends on (n, d) alone.
#include "logits_tile.h"

#include <math.h>

namespace clipfs {
namespace {

constexpr int KRR_THREADS = 256;
constexpr int KRR_MAX_D = 1024, KRR_MAX_N = 16384, KRR_MAX_C = 4096, KRR_MAX_B = 1 << 24, KRR_SMALL_N = 1024;
constexpr int KRR_MAX_NT = 8;

__device__ __forceinline__ float krr_exp(float a, float bl2) { return __builtin_amdgcn_exp2f((a - 1.f) * bl2); }

__global__ __launch_bounds__(KRR_THREADS) void krr_system_map_kernel(float* __restrict__ A, int n, int n4, int ld, float bl2,
                                                                     float lambda) {
  const int q4 = n4 >> 2;
  const size_t total = (size_t)n4 * q4;
  for (size_t e = (size_t)blockIdx.x * KRR_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * KRR_THREADS) {
    const int i = (int)(e / q4), j0 = 4 * (int)(e - (size_t)i * q4);
    f32x4* p = reinterpret_cast<f32x4*>(A + (size_t)i * ld + j0);
    f32x4 v;
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (i < n && j0 < n) v = *p;  // the product wrote [n, n]: elements past n of this float4 are not read below
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int j = j0 + x;
      float r = i == j ? 1.f : 0.f;  // the pad: identity
      if (i < n && j < n) {
        r = krr_exp(v[x], bl2);
        if (i == j) r += lambda;
      }
      v[x] = r;
    }
    *p = v;
  }
}

__global__ __launch_bounds__(KRR_THREADS) void krr_targets_kernel(const int32_t* __restrict__ labels, const float* __restrict__ baseS,
                                                                  int ldbs, float* __restrict__ Et, int n, int n4, int ldet, float t) {
  const int c = blockIdx.y;
  for (int j = blockIdx.x * KRR_THREADS + threadIdx.x; j < n4; j += gridDim.x * KRR_THREADS) {
    float v = 0.f;
    if (j < n) {
      v = labels[j] == c ? t : 0.f;
      if (baseS) v -= baseS[(size_t)j * ldbs + c];
    }
    Et[(size_t)c * ldet + j] = v;
  }
}

// LDS: sX, sS [32][132] | Ps [4][32][33] | Gs [32][32]  (54 784 bytes, static)
template <int NT>
__global__ __launch_bounds__(KRR_THREADS) void krr_apply_kernel(const float* __restrict__ X, const float* __restrict__ S,
                                                                const float* __restrict__ At, int ldat,
                                                                const float* __restrict__ base, int ldbase, float* __restrict__ out,
                                                                int ldo, int B, int n, int C, int d, float bl2) {
  __shared__ __attribute__((aligned(16))) float sX[32 * TILE_KST];
  __shared__ __attribute__((aligned(16))) float sS[32 * TILE_KST];
  __shared__ float Ps[4][32 * TILE_PS];  // per wave: [query][key] partial dot products
  __shared__ float Gs[32 * 32];          // [key][query]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * 32;
  const int cbase = blockIdx.y * (128 * NT) + 32 * w;  // this wave's class tiles: cbase + 128 a
  const int n4 = (n + 3) & ~3;
  f32x16 acc[NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
  TileStage st;
  st.load(X, x0, B, S, 0, n, d, 0, tid);
  for (int y0 = 0; y0 < n; y0 += 32) {
    const f32x16 s = tile_dots_staged(st, X, x0, B, S, y0, n, d, x0, y0 + 32, y0 + 32 < n, sX, sS, tid);
#pragma unroll
    for (int r = 0; r < 16; ++r) Ps[w][tile_row(r, h) * TILE_PS + li] = s[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + TILE_THREADS * i, own = e & 31, oth = e >> 5;
      const float a = tile_sum4(Ps, own * TILE_PS + oth);
      Gs[oth * 32 + own] = (x0 + own < B && y0 + oth < n) ? krr_exp(a, bl2) : 0.f;
    }
    __syncthreads();
    float ga[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) ga[i] = Gs[(16 * h + i) * 32 + li];
    const int k0 = y0 + 16 * h;  // this half-wave's 16 keys
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const int ct = cbase + 128 * a;
      if (ct < C) {  // wave-uniform
        const float* ar = At + (size_t)min(ct + li, C - 1) * ldat + k0;
        f32x4 av[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          av[q][0] = av[q][1] = av[q][2] = av[q][3] = 0.f;
          if (k0 + 4 * q < n4) av[q] = *reinterpret_cast<const f32x4*>(ar + 4 * q);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float v = k0 + 4 * q + x < n ? av[q][x] : 0.f;  // the sum runs over j < n whatever the pad holds
            acc[a] = tile_mfma(ga[4 * q + x], v, acc[a]);
          }
      }
    }
    // Gs and Ps are written again only after the barriers of the next tile's staged chunks
  }
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    const int c = cbase + 128 * a + li;
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int xi = x0 + tile_row(r, h);
        if (xi < B) out[(size_t)xi * ldo + c] = (base ? base[(size_t)xi * ldbase + c] : 0.f) + acc[a][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- host
typedef struct clipfs_krr_params KrrParams;
typedef struct clipfs_krr_buffers KrrBufs;
typedef struct clipfs_krr_plan KrrPlan;

int krr_check_shape(int n, int C, int d, const char* who) {
  CLIPFS_REQUIRE(d >= 4 && d <= KRR_MAX_D && d % 4 == 0, "%s: d = %d must be a multiple of 4 in [4, %d]", who, d, KRR_MAX_D);
  CLIPFS_REQUIRE(n >= 1 && n <= KRR_MAX_N, "%s: n = %d outside [1, %d]", who, n, KRR_MAX_N);
  CLIPFS_REQUIRE(C >= 1 && C <= KRR_MAX_C, "%s: C = %d outside [1, %d]", who, C, KRR_MAX_C);
  return CLIPFS_OK;
}

int krr_check_beta(float beta, const char* who) {
  CLIPFS_REQUIRE(beta > 0.f && beta <= 100.f, "%s: beta = %g outside (0, 100]", who, (double)beta);
  return CLIPFS_OK;
}

int krr_check_ptr(const void* p, unsigned mask, const char* name, const char* who) {
  CLIPFS_REQUIRE(p != nullptr, "%s: %s is NULL", who, name);
  CLIPFS_REQUIRE((reinterpret_cast<uintptr_t>(p) & mask) == 0, "%s: %s is not %u-byte aligned", who, name, mask + 1);
  return CLIPFS_OK;
}

bool krr_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

int krr_check_labels_host(const int32_t* lh, int n, int C, const char* who) {
  if (!lh) return CLIPFS_OK;
  for (int j = 0; j < n; ++j)
    CLIPFS_REQUIRE(lh[j] >= 0 && lh[j] < C, "%s: labels_host[%d] = %d outside [0, C = %d)", who, j, lh[j], C);
  return CLIPFS_OK;
}

int krr_nt(int C) {
  const int per = ((C + 31) / 32 + 3) / 4;
  return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : KRR_MAX_NT;
}

unsigned krr_grid(size_t items) {
  const size_t g = (items + KRR_THREADS - 1) / KRR_THREADS;
  return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

void krr_run_targets(const int32_t* labels, const float* baseS, int ldbs, float* Et, int n, int C, int ldet, float t, hipStream_t st) {
  const int n4 = (n + 3) & ~3;
  hipLaunchKernelGGL(krr_targets_kernel, dim3((unsigned)((n4 + KRR_THREADS - 1) / KRR_THREADS), (unsigned)C), dim3(KRR_THREADS), 0,
                     st, labels, baseS, ldbs, Et, n, n4, ldet, t);
}

int krr_run_system(const float* S, float* A, int n, int d, int ld, float beta, float lambda, void* stream) {
  clipfs_gemm_args g = {};
  g.struct_size = sizeof(g);
  g.A = S;
  g.B = S;
  g.C = A;
  g.M = g.N = n;
  g.K = d;
  g.lda = g.ldb = d;
  g.ldc = ld;
  g.alpha = 1.f;
  CLIPFS_CHECK(clipfs_gemm_nt(&g, stream));
  const int n4 = (n + 3) & ~3;
  hipLaunchKernelGGL(krr_system_map_kernel, dim3(krr_grid((size_t)n4 * (n4 >> 2))), dim3(KRR_THREADS), 0, (hipStream_t)stream, A, n,
                     n4, ld, beta * TILE_LOG2E, lambda);
  return CLIPFS_OK;
}

int krr_check_system(const float* S, float* A, int n, int d, int ld, float beta, float lambda, const char* who,
                     const char* sname = "S") {
  CLIPFS_CHECK(krr_check_shape(n, 1, d, who));
  CLIPFS_CHECK(krr_check_beta(beta, who));
  CLIPFS_REQUIRE(isfinite(lambda) && lambda > 0.f, "%s: lambda = %g must be finite and > 0", who, (double)lambda);
  const int n4 = (n + 3) & ~3;
  CLIPFS_REQUIRE(ld >= n4 && ld % 4 == 0, "%s: ld = %d must be a multiple of 4 and >= n4 = %d", who, ld, n4);
  CLIPFS_CHECK(krr_check_ptr(S, 15u, sname, who));
  CLIPFS_CHECK(krr_check_ptr(A, 15u, "A", who));
  CLIPFS_REQUIRE(!krr_overlap(S, (size_t)n * d * 4, A, ((size_t)(n4 - 1) * ld + n4) * 4), "%s: A %s %s", who,
                 sname[0] == 'S' ? "overlaps" : "aliases", sname);
  return CLIPFS_OK;
}

int krr_check_targets(const int32_t* labels, const int32_t* labels_host, const float* baseS, int ldbs, float* Et, int n, int C,
                      int ldet, float t, const char* who) {
  CLIPFS_CHECK(krr_check_shape(n, C, 4, who));
  CLIPFS_REQUIRE(isfinite(t), "%s: t = %g must be finite", who, (double)t);
  const int n4 = (n + 3) & ~3;
  CLIPFS_REQUIRE(ldet >= n4 && ldet % 4 == 0, "%s: ldet = %d must be a multiple of 4 and >= n4 = %d", who, ldet, n4);
  CLIPFS_CHECK(krr_check_ptr(labels, 3u, "labels", who));
  CLIPFS_CHECK(krr_check_ptr(Et, 15u, "Et", who));
  if (baseS) {
    CLIPFS_CHECK(krr_check_ptr(baseS, 3u, "base_S", who));
    CLIPFS_REQUIRE(ldbs >= C, "%s: ldbs = %d below C = %d", who, ldbs, C);
    CLIPFS_REQUIRE(!krr_overlap(baseS, ((size_t)(n - 1) * ldbs + C) * 4, Et, ((size_t)(C - 1) * ldet + n4) * 4),
                   "%s: Et overlaps base_S", who);
  }
  CLIPFS_CHECK(krr_check_labels_host(labels_host, n, C, who));
  return CLIPFS_OK;
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_krr_plan(int n, int C, int d, int B, int panel, struct clipfs_krr_plan* plan) {
  const char* who = "clipfs_krr_plan";
  CLIPFS_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  CLIPFS_CHECK(krr_check_shape(n, C, d, who));
  CLIPFS_REQUIRE(B >= 1 && B <= KRR_MAX_B, "%s: B = %d outside [1, 2^24]", who, B);
  KrrPlan p = {};
  p.n4 = (n + 3) & ~3;
  p.panelled = p.n4 > KRR_SMALL_N ? 1 : 0;
  unsigned solver_lds = 0;
  if (p.panelled) {
    struct clipfs_spd_panels_plan sp;
    CLIPFS_CHECK(clipfs_spd_panels_plan(p.n4, C, panel, &sp));
    p.factor_launches = sp.factor_launches + sp.factor_gemms;
    p.solve_launches = sp.solve_launches + sp.solve_gemms;
    solver_lds = sp.lds_bytes;
  } else {
    CLIPFS_REQUIRE(panel >= 32 && panel <= 1024 && panel % 32 == 0, "%s: panel = %d must be a multiple of 32 in [32, 1024]", who,
                   panel);
    struct clipfs_spd_plan sp;
    CLIPFS_CHECK(clipfs_spd_plan(p.n4, C, &sp));
    p.factor_launches = sp.factor_launches;
    p.solve_launches = sp.solve_launches;
    solver_lds = sp.lds_bytes;
  }
  p.fit_launches = 3 + p.factor_launches + p.solve_launches;  // the Gram product, the map, the targets
  p.tiles_per_wave = krr_nt(C);
  p.class_chunk = 128 * p.tiles_per_wave;
  p.apply_grid_x = (unsigned)((B + 31) / 32);
  p.apply_grid_y = (unsigned)((C + p.class_chunk - 1) / p.class_chunk);
  p.threads = KRR_THREADS;
  const unsigned apply_lds = (unsigned)((2 * 32 * TILE_KST + 4 * 32 * TILE_PS + 32 * 32) * sizeof(float));
  p.lds_bytes = solver_lds > apply_lds ? solver_lds : apply_lds;
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_krr_system(const float* S, float* A, int n, int d, int ld, float beta, float lambda, void* stream) {
  CLIPFS_CHECK(krr_check_system(S, A, n, d, ld, beta, lambda, "clipfs_krr_system"));
  CLIPFS_CHECK(krr_run_system(S, A, n, d, ld, beta, lambda, stream));
  return launch_status();
}

extern "C" int clipfs_krr_targets(const int32_t* labels, const int32_t* labels_host, const float* base_S, int ldbs, float* Et,
                                  int n, int C, int ldet, float t, void* stream) {
  CLIPFS_CHECK(krr_check_targets(labels, labels_host, base_S, ldbs, Et, n, C, ldet, t, "clipfs_krr_targets"));
  krr_run_targets(labels, base_S, ldbs, Et, n, C, ldet, t, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_krr_apply(const float* X, const float* S, const float* At, int ldat, const float* base, int ldbase, float* out,
                                int ldo, int B, int n, int C, int d, float beta, void* stream) {
  const char* who = "clipfs_krr_apply";
  CLIPFS_CHECK(krr_check_shape(n, C, d, who));
  CLIPFS_REQUIRE(B >= 1 && B <= KRR_MAX_B, "%s: B = %d outside [1, 2^24]", who, B);
  CLIPFS_CHECK(krr_check_beta(beta, who));
  const int n4 = (n + 3) & ~3;
  CLIPFS_REQUIRE(ldat >= n4 && ldat % 4 == 0, "%s: ldat = %d must be a multiple of 4 and >= n4 = %d", who, ldat, n4);
  CLIPFS_REQUIRE(ldo >= C, "%s: ldo = %d below C = %d", who, ldo, C);
  CLIPFS_CHECK(krr_check_ptr(X, 15u, "X", who));
  CLIPFS_CHECK(krr_check_ptr(S, 15u, "S", who));
  CLIPFS_CHECK(krr_check_ptr(At, 15u, "At", who));
  CLIPFS_CHECK(krr_check_ptr(out, 3u, "out", who));
  const size_t so = ((size_t)(B - 1) * ldo + C) * 4;
  if (base) {
    CLIPFS_CHECK(krr_check_ptr(base, 3u, "base", who));
    CLIPFS_REQUIRE(ldbase >= C, "%s: ldbase = %d below C = %d", who, ldbase, C);
    CLIPFS_REQUIRE(!krr_overlap(base, ((size_t)(B - 1) * ldbase + C) * 4, out, so), "%s: out overlaps base", who);
  }
  CLIPFS_REQUIRE(!krr_overlap(X, (size_t)B * d * 4, out, so) && !krr_overlap(S, (size_t)n * d * 4, out, so) &&
                     !krr_overlap(At, ((size_t)(C - 1) * ldat + n4) * 4, out, so),
                 "%s: out overlaps X, S or At", who);
  const int nt = krr_nt(C);
  const dim3 grid((unsigned)((B + 31) / 32), (unsigned)((C + 128 * nt - 1) / (128 * nt)));
  const float bl2 = beta * TILE_LOG2E;
  hipStream_t st = (hipStream_t)stream;
#define KRR_APPLY(NT_) \
  hipLaunchKernelGGL((krr_apply_kernel<NT_>), grid, dim3(KRR_THREADS), 0, st, X, S, At, ldat, base, ldbase, out, ldo, B, n, C, d, bl2)
  if (nt == 1) KRR_APPLY(1);
  else if (nt == 2) KRR_APPLY(2);
  else if (nt == 4) KRR_APPLY(4);
  else KRR_APPLY(8);
#undef KRR_APPLY
  return launch_status();
}

extern "C" int clipfs_krr_fit(const struct clipfs_krr_params* p, const struct clipfs_krr_buffers* b, void* stream) {
  const char* who = "clipfs_krr_fit";
  CLIPFS_REQUIRE(p != nullptr, "%s: NULL params", who);
  CLIPFS_REQUIRE(p->struct_size == sizeof(KrrParams), "%s: params.struct_size = %u, this library expects %u", who, p->struct_size,
                 (unsigned)sizeof(KrrParams));
  CLIPFS_REQUIRE(b != nullptr, "%s: NULL buffers", who);
  CLIPFS_REQUIRE(b->struct_size == sizeof(KrrBufs), "%s: buffers.struct_size = %u, this library expects %u", who, b->struct_size,
                 (unsigned)sizeof(KrrBufs));
  KrrPlan pl;
  CLIPFS_CHECK(clipfs_krr_plan(p->n, p->C, p->d, 1, p->panel, &pl));
  const int n = p->n, C = p->C, d = p->d, n4 = pl.n4;
  CLIPFS_CHECK(krr_check_system(b->shots, b->A, n, d, n4, p->beta, p->lambda, who, "shots"));
  CLIPFS_CHECK(krr_check_targets(b->labels, b->labels_host, b->base_S, b->ldbs, b->Et, n, C, n4, p->t, who));
  CLIPFS_CHECK(krr_check_ptr(b->chol, 15u, "chol", who));
  CLIPFS_CHECK(krr_check_ptr(b->info, 3u, "info", who));
  CLIPFS_CHECK(krr_check_ptr(b->At, 15u, "At", who));
  {  // a written member may not overlap another member (chol == A and At == Et aside)
    const size_t sq = (size_t)n4 * n4 * 4, rc = (size_t)C * n4 * 4;
    struct Span {
      const char* name;
      const void* ptr;
      size_t bytes;
      bool written;
    };
    const Span s[] = {{"shots", b->shots, (size_t)n * d * 4, false}, {"labels", b->labels, (size_t)n * 4, false},
                      {"base_S", b->base_S, b->base_S ? ((size_t)(n - 1) * b->ldbs + C) * 4 : 0, false},
                      {"A", b->A, sq, true}, {"chol", b->chol, sq, true}, {"info", b->info, 4, true},
                      {"Et", b->Et, rc, true}, {"At", b->At, rc, true}};
    const int ns = (int)(sizeof(s) / sizeof(s[0]));
    for (int i = 0; i < ns; ++i)
      for (int j = 0; j < ns; ++j) {
        if (i == j || !s[i].written || !s[j].ptr || s[j].bytes == 0) continue;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        if (((lo == 3 && hi == 4) || (lo == 6 && hi == 7)) && s[i].ptr == s[j].ptr) continue;  // in place
        CLIPFS_REQUIRE(!krr_overlap(s[i].ptr, s[i].bytes, s[j].ptr, s[j].bytes), "%s: %s aliases %s", who, s[i].name, s[j].name);
      }
  }
  CLIPFS_CHECK(krr_run_system(b->shots, b->A, n, d, n4, p->beta, p->lambda, stream));
  krr_run_targets(b->labels, b->base_S, b->ldbs, b->Et, n, C, n4, p->t, (hipStream_t)stream);
  if (pl.panelled) {
    CLIPFS_CHECK(clipfs_spd_factor_panels(b->A, n4, b->chol, n4, n4, p->panel, b->info, stream));
    CLIPFS_CHECK(clipfs_spd_solve_panels(b->chol, n4, n4, p->panel, b->Et, n4, b->At, n4, C, 1.f, stream));
  } else {
    CLIPFS_CHECK(clipfs_spd_factor(b->A, n4, b->chol, n4, n4, b->info, stream));
    CLIPFS_CHECK(clipfs_spd_solve(b->chol, n4, n4, b->Et, n4, b->At, n4, C, 1.f, stream));
  }
  return launch_status();
}
