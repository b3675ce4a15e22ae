// Training-free Gaussian discriminant head (clipfs.h "GDA"; Wang et al., "A Hard-to-Beat Baseline for Training-Free
// CLIP-Based Adaptation", ICLR 2024), fp32: class means and ONE shared full covariance of the few-shot features, shrunk
// towards its trace, W = d A^-1 mu by the Cholesky factor and solve of spd.hip.
//
//   stats    one workgroup per class, one thread per feature: mu_c (the class's shots summed in row order, divided by
//            n_c) and the class's columns of xt = (S - mu_y)^T [d, Mp]; workgroup 0 also zeroes the tail columns M .. Mp.
//   gram     clipfs_gemm_nt: gram = xt xt^T (K = Mp is a multiple of 32)
//   shrink   one workgroup: tau = trace(gram) in double (256 strided partial sums added in thread order), then
//            gram_ii += (float)(shrink tau / (M - 1))
//   factor   clipfs_spd_factor: gram -> chol, info
//   solve    clipfs_spd_solve: W = d chol^-1 mu
//   bias     one wave per class: b_c = log pi_c - 1/2 mu_c . W_c
//   search   one workgroup per 32 rows of g = F W^T + b, one wave per row at a time: for every alpha the row's
//            argmax_c (base + alpha g), ties to the lower class; hits are counted in LDS integers and added to `hits`
//            with integer atomics (the entry point zeroes `hits` on the stream first).
//
// No float atomics; every sum runs in an order fixed by the shapes; nothing returns to the host.
#include "logits_tile.h"

#include <limits.h>
#include <math.h>

namespace clipfs {
namespace {

constexpr int GDA_THREADS = 256;
constexpr int GDA_MAX_D = 1024, GDA_MAX_C = 4096, GDA_MAX_M = 65536, GDA_MAX_ALPHAS = 1024;
constexpr int GDA_SEARCH_ROWS = 32;

__device__ __forceinline__ int gda_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ int gda_wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(GDA_THREADS) void gda_stats_kernel(const float* __restrict__ S, const int32_t* __restrict__ off,
                                                                float* __restrict__ mu, float* __restrict__ xt, int M, int Mp,
                                                                int d) {
  const int c = blockIdx.x, tid = threadIdx.x;
  // offsets are checked on the host copy; whatever the device copy holds, nothing leaves [0, M)
  const int lo = gda_clampi(off[c], 0, M), hi = gda_clampi(off[c + 1], lo, M);
  const float nc = (float)(hi - lo);
  for (int dd = tid; dd < d; dd += GDA_THREADS) {
    float acc = 0.f;
    for (int m = lo; m < hi; ++m) acc += S[(size_t)m * d + dd];
    const float mean = hi > lo ? acc / nc : 0.f;
    mu[(size_t)c * d + dd] = mean;
    float* xr = xt + (size_t)dd * Mp;
    for (int m = lo; m < hi; ++m) xr[m] = S[(size_t)m * d + dd] - mean;
    if (c == 0)
      for (int m = M; m < Mp; ++m) xr[m] = 0.f;
  }
}

__global__ __launch_bounds__(GDA_THREADS) void gda_shrink_kernel(float* __restrict__ G, float* __restrict__ tau_out, int d,
                                                                 double scale) {
  __shared__ double part[GDA_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < d; i += GDA_THREADS) s += (double)G[(size_t)i * d + i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int t = 0; t < GDA_THREADS; ++t) tot += part[t];
    part[0] = tot;
    *tau_out = (float)tot;
  }
  __syncthreads();
  const float ridge = (float)(scale * part[0]);
  for (int i = tid; i < d; i += GDA_THREADS) G[(size_t)i * d + i] = G[(size_t)i * d + i] + ridge;
}

__global__ __launch_bounds__(GDA_THREADS) void gda_bias_kernel(const float* __restrict__ mu, const float* __restrict__ W,
                                                               const int32_t* __restrict__ off, float* __restrict__ b, int C, int d,
                                                               int M, int prior) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * (GDA_THREADS / 64) + (threadIdx.x >> 6);
  if (c >= C) return;  // wave-uniform; no barrier in this kernel
  float acc = 0.f;
  for (int dd = lane; dd < d; dd += 64) acc += mu[(size_t)c * d + dd] * W[(size_t)c * d + dd];
  acc = wave_sum(acc);
  if (lane == 0) {
    double lp = -log((double)C);
    if (prior == 1) {
      const int lo = gda_clampi(off[c], 0, M), hi = gda_clampi(off[c + 1], lo, M);
      lp = log((double)(hi - lo) / (double)M);
    }
    b[c] = (float)lp - 0.5f * acc;
  }
}

__global__ __launch_bounds__(GDA_THREADS) void gda_search_kernel(const float* __restrict__ g, const float* __restrict__ base,
                                                                 int ldbase, const int64_t* __restrict__ target,
                                                                 const float* __restrict__ alphas, int32_t* __restrict__ hits, int B,
                                                                 int C, int nA) {
  __shared__ int cnt[GDA_MAX_ALPHAS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int a = tid; a < nA; a += GDA_THREADS) cnt[a] = 0;
  __syncthreads();
  for (int rr = w; rr < GDA_SEARCH_ROWS; rr += GDA_THREADS / 64) {
    const int row = blockIdx.x * GDA_SEARCH_ROWS + rr;
    if (row >= B) break;  // wave-uniform; the barrier below is outside the loop
    const float* gr = g + (size_t)row * C;
    const float* br = base ? base + (size_t)row * ldbase : nullptr;
    const int64_t tgt = target[row];
    for (int a = 0; a < nA; ++a) {
      const float al = alphas[a];
      float bv = -INFINITY;
      int bc = INT_MAX;
      for (int c = lane; c < C; c += 64) {
        const float v = (br ? br[c] : 0.f) + al * gr[c];
        if (v > bv) {  // ascending c: the first of equals stays
          bv = v;
          bc = c;
        }
      }
      const float bm = wave_max(bv);
      int best = gda_wave_min_int(bv == bm ? bc : INT_MAX);
      if (best >= C) best = 0;  // a row that is not numbers: class 0
      if (lane == 0 && (int64_t)best == tgt) atomicAdd(&cnt[a], 1);  // an LDS integer
    }
  }
  __syncthreads();
  for (int a = tid; a < nA; a += GDA_THREADS)
    if (cnt[a]) atomicAdd(&hits[a], cnt[a]);  // integers: the total does not depend on the order
}

// ------------------------------------------------------------------------------------------------- host
typedef struct clipfs_gda_params GdaParams;
typedef struct clipfs_gda_buffers GdaBufs;
typedef struct clipfs_gda_plan GdaPlan;

int gda_check_params(const GdaParams* p, const char* who) {
  CLIPFS_REQUIRE(p != nullptr, "%s: NULL params", who);
  CLIPFS_REQUIRE(p->struct_size == sizeof(GdaParams), "%s: params.struct_size = %u, this library expects %u", who, p->struct_size,
                 (unsigned)sizeof(GdaParams));
  CLIPFS_REQUIRE(p->d >= 4 && p->d <= GDA_MAX_D && p->d % 4 == 0, "%s: d = %d must be a multiple of 4 in [4, %d]", who, p->d,
                 GDA_MAX_D);
  CLIPFS_REQUIRE(p->C >= 1 && p->C <= GDA_MAX_C, "%s: C = %d outside [1, %d]", who, p->C, GDA_MAX_C);
  CLIPFS_REQUIRE(p->M >= 2 && p->M <= GDA_MAX_M, "%s: M = %d outside [2, %d]", who, p->M, GDA_MAX_M);
  CLIPFS_REQUIRE(p->M >= p->C, "%s: M = %d below C = %d (every class owns at least one shot)", who, p->M, p->C);
  CLIPFS_REQUIRE(p->prior == CLIPFS_GDA_PRIOR_UNIFORM || p->prior == CLIPFS_GDA_PRIOR_EMPIRICAL,
                 "%s: prior = %d is neither CLIPFS_GDA_PRIOR_UNIFORM nor CLIPFS_GDA_PRIOR_EMPIRICAL", who, p->prior);
  CLIPFS_REQUIRE(isfinite(p->shrink) && p->shrink >= 0.f, "%s: shrink = %g must be finite and >= 0", who, (double)p->shrink);
  return CLIPFS_OK;
}

int gda_check_bufs(const GdaBufs* b, const char* who) {
  CLIPFS_REQUIRE(b != nullptr, "%s: NULL buffers", who);
  CLIPFS_REQUIRE(b->struct_size == sizeof(GdaBufs), "%s: buffers.struct_size = %u, this library expects %u", who, b->struct_size,
                 (unsigned)sizeof(GdaBufs));
  return CLIPFS_OK;
}

struct GdaSpan {
  const char* name;
  const void* p;
  size_t bytes;
  bool written, align16;
};

enum GdaField { GF_SHOTS, GF_OFFSETS, GF_MU, GF_XT, GF_GRAM, GF_TAU, GF_CHOL, GF_INFO, GF_W, GF_B, GF_COUNT };
#define GF(x) (1u << GF_##x)

int gda_spans(const GdaParams* p, int Mp, const GdaBufs* b, unsigned used, unsigned written, const char* who) {
  const size_t M = p->M, C = p->C, d = p->d;
  const GdaSpan all[GF_COUNT] = {
      {"shots", b->shots, M * d * 4, false, true},  {"offsets", b->offsets, (C + 1) * 4, false, false},
      {"mu", b->mu, C * d * 4, false, true},        {"xt", b->xt, d * (size_t)Mp * 4, false, true},
      {"gram", b->gram, d * d * 4, false, true},    {"tau", b->tau, 4, false, false},
      {"chol", b->chol, d * d * 4, false, true},    {"info", b->info, 4, false, false},
      {"W", b->W, C * d * 4, false, true},          {"b", b->b, C * 4, false, false},
  };
  GdaSpan s[GF_COUNT];
  int n = 0;
  for (int f = 0; f < GF_COUNT; ++f)
    if (used & (1u << f)) {
      s[n] = all[f];
      s[n].written = (written & (1u << f)) != 0;
      ++n;
    }
  for (int i = 0; i < n; ++i) {
    CLIPFS_REQUIRE(s[i].p != nullptr, "%s: %s is NULL", who, s[i].name);
    const uintptr_t a = reinterpret_cast<uintptr_t>(s[i].p);
    CLIPFS_REQUIRE((a & (s[i].align16 ? 15u : 3u)) == 0, "%s: %s is not %d-byte aligned", who, s[i].name, s[i].align16 ? 16 : 4);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      if (i == j || !s[i].written) continue;
      const uintptr_t a = reinterpret_cast<uintptr_t>(s[i].p), c = reinterpret_cast<uintptr_t>(s[j].p);
      CLIPFS_REQUIRE(!(a < c + s[j].bytes && c < a + s[i].bytes), "%s: %s aliases %s", who, s[i].name, s[j].name);
    }
  return CLIPFS_OK;
}

// the host copy of the offsets, when given: 0 = offsets[0] < offsets[1] < ... < offsets[C] = M
int gda_check_offsets(const GdaParams* p, const GdaBufs* b, const char* who) {
  const int32_t* o = b->offsets_host;
  if (!o) return CLIPFS_OK;
  CLIPFS_REQUIRE(o[0] == 0, "%s: offsets[0] = %d must be 0", who, o[0]);
  for (int c = 0; c < p->C; ++c) {
    CLIPFS_REQUIRE(o[c + 1] != o[c], "%s: offsets: class %d owns no shot (offsets[%d] = offsets[%d] = %d)", who, c, c, c + 1, o[c]);
    CLIPFS_REQUIRE(o[c + 1] > o[c], "%s: offsets[%d] = %d is below offsets[%d] = %d", who, c + 1, o[c + 1], c, o[c]);
  }
  CLIPFS_REQUIRE(o[p->C] == p->M, "%s: offsets[C] = %d must be M = %d", who, o[p->C], p->M);
  return CLIPFS_OK;
}

void gda_run_stats(const GdaParams* p, const GdaPlan& pl, const GdaBufs* b, hipStream_t st) {
  hipLaunchKernelGGL(gda_stats_kernel, dim3(pl.stats_grid), dim3(GDA_THREADS), 0, st, b->shots, b->offsets, b->mu, b->xt, p->M, pl.Mp,
                     p->d);
}

void gda_run_shrink(const GdaParams* p, const GdaBufs* b, hipStream_t st) {
  hipLaunchKernelGGL(gda_shrink_kernel, dim3(1), dim3(GDA_THREADS), 0, st, b->gram, b->tau, p->d,
                     (double)p->shrink / (double)(p->M - 1));
}

void gda_run_bias(const GdaParams* p, const GdaPlan& pl, const GdaBufs* b, hipStream_t st) {
  hipLaunchKernelGGL(gda_bias_kernel, dim3(pl.bias_grid), dim3(GDA_THREADS), 0, st, (const float*)b->mu, (const float*)b->W,
                     b->offsets, b->b, p->C, p->d, p->M, p->prior);
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_gda_plan(const struct clipfs_gda_params* params, struct clipfs_gda_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_gda_plan: NULL plan");
  CLIPFS_CHECK(gda_check_params(params, "clipfs_gda_plan"));
  struct clipfs_spd_plan sp;
  CLIPFS_CHECK(clipfs_spd_plan(params->d, params->C, &sp));
  GdaPlan p = {};
  p.Mp = (params->M + 31) / 32 * 32;
  p.factor_launches = sp.factor_launches;
  p.solve_launches = sp.solve_launches;
  p.launches = 4 + sp.factor_launches + sp.solve_launches;  // stats, gram, shrink, bias + the factor and the solve
  p.stats_grid = (unsigned)params->C;
  p.bias_grid = (unsigned)((params->C + 3) / 4);
  p.solve_grid = sp.solve_grid;
  p.threads = GDA_THREADS;
  p.lds_bytes = sp.lds_bytes;  // the solve's rows; stats, shrink and bias hold at most 2 KB
  p.xt_floats = (size_t)params->d * p.Mp;
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_gda_stats(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* b, void* stream) {
  const char* who = "clipfs_gda_stats";
  GdaPlan pl;
  CLIPFS_CHECK(clipfs_gda_plan(params, &pl));
  CLIPFS_CHECK(gda_check_bufs(b, who));
  CLIPFS_CHECK(gda_spans(params, pl.Mp, b, GF(SHOTS) | GF(OFFSETS) | GF(MU) | GF(XT), GF(MU) | GF(XT), who));
  CLIPFS_CHECK(gda_check_offsets(params, b, who));
  gda_run_stats(params, pl, b, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_gda_shrink(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* b, void* stream) {
  const char* who = "clipfs_gda_shrink";
  GdaPlan pl;
  CLIPFS_CHECK(clipfs_gda_plan(params, &pl));
  CLIPFS_CHECK(gda_check_bufs(b, who));
  CLIPFS_CHECK(gda_spans(params, pl.Mp, b, GF(GRAM) | GF(TAU), GF(GRAM) | GF(TAU), who));
  gda_run_shrink(params, b, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_gda_bias(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* b, void* stream) {
  const char* who = "clipfs_gda_bias";
  GdaPlan pl;
  CLIPFS_CHECK(clipfs_gda_plan(params, &pl));
  CLIPFS_CHECK(gda_check_bufs(b, who));
  CLIPFS_CHECK(gda_spans(params, pl.Mp, b, GF(OFFSETS) | GF(MU) | GF(W) | GF(B), GF(B), who));
  CLIPFS_CHECK(gda_check_offsets(params, b, who));
  gda_run_bias(params, pl, b, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_gda_search(const float* g, const float* base, int ldbase, const int64_t* target, const float* alphas,
                                 int32_t* hits, int B, int C, int nA, void* stream) {
  const char* who = "clipfs_gda_search";
  CLIPFS_REQUIRE(B >= 1 && B <= (1 << 24), "%s: B = %d outside [1, 2^24]", who, B);
  CLIPFS_REQUIRE(C >= 1 && C <= GDA_MAX_C, "%s: C = %d outside [1, %d]", who, C, GDA_MAX_C);
  CLIPFS_REQUIRE(nA >= 1 && nA <= GDA_MAX_ALPHAS, "%s: nA = %d outside [1, %d]", who, nA, GDA_MAX_ALPHAS);
  CLIPFS_REQUIRE(g != nullptr, "%s: g is NULL", who);
  CLIPFS_REQUIRE(target != nullptr, "%s: target is NULL", who);
  CLIPFS_REQUIRE(alphas != nullptr, "%s: alphas is NULL", who);
  CLIPFS_REQUIRE(hits != nullptr, "%s: hits is NULL", who);
  CLIPFS_REQUIRE(!base || ldbase >= C, "%s: ldbase = %d below C = %d", who, ldbase, C);
  CLIPFS_REQUIRE(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(alphas) |
                   reinterpret_cast<uintptr_t>(hits)) & 3u) == 0 && (reinterpret_cast<uintptr_t>(target) & 7u) == 0,
                 "%s: g, base, alphas or hits is not 4-byte aligned, or target not 8-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(hits, 0, (size_t)nA * sizeof(int32_t), st);
  if (e != hipSuccess) {
    set_error("%s: hipMemsetAsync failed: %s", who, hipGetErrorString(e));
    return CLIPFS_HIPERR_BASE + (int)e;
  }
  hipLaunchKernelGGL(gda_search_kernel, dim3((unsigned)((B + GDA_SEARCH_ROWS - 1) / GDA_SEARCH_ROWS)), dim3(GDA_THREADS), 0, st, g,
                     base, ldbase, target, alphas, hits, B, C, nA);
  return launch_status();
}

extern "C" int clipfs_gda_fit(const struct clipfs_gda_params* params, const struct clipfs_gda_buffers* b, void* stream) {
  const char* who = "clipfs_gda_fit";
  GdaPlan pl;
  CLIPFS_CHECK(clipfs_gda_plan(params, &pl));
  CLIPFS_CHECK(gda_check_bufs(b, who));
  const unsigned all = (1u << GF_COUNT) - 1u;
  CLIPFS_CHECK(gda_spans(params, pl.Mp, b, all, all & ~(GF(SHOTS) | GF(OFFSETS)), who));
  CLIPFS_CHECK(gda_check_offsets(params, b, who));
  hipStream_t st = (hipStream_t)stream;
  const int d = params->d;
  gda_run_stats(params, pl, b, st);
  clipfs_gemm_args ga = {};
  ga.struct_size = sizeof(ga);
  ga.A = b->xt;
  ga.B = b->xt;
  ga.C = b->gram;
  ga.M = ga.N = d;
  ga.K = pl.Mp;
  ga.lda = ga.ldb = pl.Mp;
  ga.ldc = d;
  ga.alpha = 1.f;
  CLIPFS_CHECK(clipfs_gemm_nt(&ga, stream));
  gda_run_shrink(params, b, st);
  CLIPFS_CHECK(clipfs_spd_factor(b->gram, d, b->chol, d, d, b->info, stream));
  CLIPFS_CHECK(clipfs_spd_solve(b->chol, d, d, b->mu, d, b->W, d, params->C, (float)d, stream));
  gda_run_bias(params, pl, b, st);
  return launch_status();
}
