// Symmetric positive definite systems in fp32 (clipfs.h "SPD"): a blocked Cholesky factor A = L L^T and the solve
// X[i, :] = alpha A^-1 R[i, :] for many right-hand sides, block 32 on v_mfma_f32_32x32x2_f32 (tile_dots_ld of
// logits_tile.h).  n is a multiple of 4 in [4, 1024]; a last block of fewer than 32 columns is padded ON CHIP with the
// identity (pad pivots are 1, pad products are discarded), never in memory.
//
//   factor   left-looking, ONE launch per block column j, one workgroup per 32-row tile (i, j) at or below the diagonal.
//            Every workgroup forms the updated diagonal tile D = A_jj - L[j, :j] L[j, :j]^T itself (the four waves split
//            the columns in 64-column steps, their partials are added in wave order) and wave 0 factors it in
//            registers: lane r owns row r, the pivot column travels by v_readlane.  That is 32 sequential steps of
//            32 x 32 work, repeated in every workgroup, instead of a launch of its own and a grid-wide dependency.  The
//            workgroup then forms its own tile T = A_ij - L[i, :j] L[j, :j]^T and wave 0 applies L_jj^-T, one lane per
//            row.  It writes L_ij and, transposed, the strict upper tile (j, i).
//            The diagonal tile (j, j) is NOT written in launch j: with L == A the other workgroups of that launch are
//            still reading A_jj.  Launch j + 1 carries one more workgroup that forms and factors tile (j, j) again
//            (bitwise the same numbers: the same code on the same inputs) and writes it; the last launch has the diagonal
//            workgroup alone in its block row and writes its tile itself.  So the factor is ceil(n / 32) launches, in
//            place or not, and in place IS out of place bit for bit.
//   info     the diagonal workgroup of launch j reports the first pivot of its block that is <= 0 or not finite
//            (1-based, global) unless an earlier launch reported one; launch 0 writes 0 on success.  Column k of a tile
//            depends on the columns before it only, so everything before the reported pivot is valid.  Nothing loops on
//            data and nothing is indexed by a computed value: the call always terminates.
//   solve    two launches, forward (Y L^T = R) and backward (X L = Y).  One workgroup owns 32 right-hand-side rows, keeps
//            them in LDS (32 x (n + 4) floats: 128.5 KB at n = 1024) and walks the block columns itself: the part already
//            solved times the block's rows of L (forward: the lower triangle; backward: the transposed copy in the strict
//            upper triangle, so both read contiguous rows) on the matrix cores, then the 32 x 32 substitution in
//            registers, one lane per row.  The forward launch leaves Y in X.
//   panels   the same contract for n up to 16384 (clipfs_spd_factor_panels / clipfs_spd_solve_panels, at the end of this
//            file), right-looking over panels of `panel` <= 1024 columns, built from the kernels above on sub-matrix
//            views: the diagonal block by the factor kernel (its info reports carried to global columns by `base`, never
//            overwritten by a later panel under `keep`), L21 = A21 L11^-T by the FORWARD solve launch alone with the rows
//            of A21 as right-hand sides, L21 mirrored above the diagonal, A22 -= L21 L21^T by clipfs_gemm_nt in row
//            bands that stop at their own last row.  The solve substitutes on a diagonal block (one-directional launch)
//            and takes the panel's part out of every remaining column with one clipfs_gemm_nt call; the right-hand sides
//            live in X, a last launch scales by alpha.
//
// No atomics at all; every output element is written by one thread; the order of every sum depends on n alone.
#include "logits_tile.h"

#include <float.h>
#include <math.h>

namespace clipfs {
namespace {

constexpr int SPD_THREADS = 256, SPD_B = 32, SPD_TS = 33;  // TS: row stride of a 32 x 32 tile in LDS
constexpr int SPD_MAX_N = 1024, SPD_MAX_RHS = 65536;
constexpr int SPD_YPAD = 4;  // the right-hand-side rows in LDS: stride n + 4 (16-byte rows)

__device__ __forceinline__ float spd_lane(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// Cholesky of the tile in Ds (lower triangle read, lower triangle written), by one wave: lane (r = lane & 31) owns row r.
// Returns 0, or the 1-based index of the first pivot <= 0 or not finite (the same value in every lane).
__device__ __forceinline__ int spd_chol32(float* Ds, int lane) {
  const int r = lane & 31;
  float row[SPD_B];
#pragma unroll
  for (int c = 0; c < SPD_B; ++c) row[c] = Ds[r * SPD_TS + c];
  int bad = 0;
#pragma unroll
  for (int k = 0; k < SPD_B; ++k) {
    const float p = spd_lane(row[k], k);
    if (bad == 0 && !(p > 0.f && p <= FLT_MAX)) bad = k + 1;
    const float l = sqrtf(p);
    const float v = r == k ? l : row[k] / l;  // rows above k hold nothing that is read
    row[k] = v;
#pragma unroll
    for (int c = k + 1; c < SPD_B; ++c) row[c] -= v * spd_lane(v, c);
  }
  if (lane < 32) {
#pragma unroll
    for (int c = 0; c < SPD_B; ++c) Ds[r * SPD_TS + c] = row[c];
  }
  return bad;
}

// t <- t Ls^-T (forward: y L^T = t) or t <- t Ls^-1 (backward: x L = t) for the lower triangular tile Ls; t is one row
// of right-hand sides per lane.  The coefficients are the same for every lane: lane k loads row k of Ls once and
// Ls[k][c] travels by v_readlane (as 528 LDS reads the compiler hoisted them all and spilled).  Column k of the forward
// form needs the columns before it only.
template <bool BACK>
__device__ __forceinline__ void spd_subst32(float (&t)[SPD_B], const float* Ls, int lane) {
  float lr[SPD_B];
#pragma unroll
  for (int c = 0; c < SPD_B; ++c) lr[c] = Ls[(lane & 31) * SPD_TS + c];
  if (!BACK) {
#pragma unroll
    for (int k = 0; k < SPD_B; ++k) {
      float s = t[k];
#pragma unroll
      for (int c = 0; c < k; ++c) s -= t[c] * spd_lane(lr[c], k);
      t[k] = s / spd_lane(lr[k], k);
    }
  } else {
#pragma unroll
    for (int k = SPD_B - 1; k >= 0; --k) {
      const float x = t[k] / spd_lane(lr[k], k);
      t[k] = x;
#pragma unroll
      for (int c = 0; c < k; ++c) t[c] -= x * spd_lane(lr[c], k);
    }
  }
}

__device__ __forceinline__ float spd_sum4(const float* Ps, int at) {
  return ((Ps[at] + Ps[32 * SPD_TS + at]) + Ps[2 * 32 * SPD_TS + at]) + Ps[3 * 32 * SPD_TS + at];
}

// ------------------------------------------------------------------------------------------------- factor
// Launch j: workgroups 0 .. nb - j - 1 own the tiles (j + x, j); with j > 0 workgroup nb - j forms, factors and writes
// the diagonal tile (j - 1, j - 1).  A and L may be the same memory.
// `base`, `keep`: the block is the diagonal block of a larger matrix (the panelled factor below) whose first column is
// `base`, and with `keep` launch 0 leaves an earlier panel's report alone.  (0, 0) is the whole-matrix call.
__global__ __launch_bounds__(SPD_THREADS) void spd_factor_kernel(const float* A, int lda, float* L, int ldl, int n, int j,
                                                                 int32_t* info, int base, int keep) {
  __shared__ float PsD[4 * 32 * SPD_TS];
  __shared__ float PsT[4 * 32 * SPD_TS];
  __shared__ float Ds[32 * SPD_TS];
  __shared__ float Ts[32 * SPD_TS];
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int nb = (n + SPD_B - 1) / SPD_B;
  const bool finish = (int)blockIdx.x == nb - j;
  const int jj = finish ? j - 1 : j, i = finish ? j - 1 : j + (int)blockIdx.x;
  const int cj = SPD_B * jj, ci = SPD_B * i, K = cj;  // K: the columns already factored
  const bool diag = i == jj;
  {
    const f32x16 acc = tile_dots_ld(L, ldl, cj, n, L, ldl, cj, n, K, 64 * w, 256, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) PsD[w * 32 * SPD_TS + tile_row(r, h) * SPD_TS + li] = acc[r];
  }
  if (!diag) {  // workgroup-uniform
    const f32x16 acc = tile_dots_ld(L, ldl, ci, n, L, ldl, cj, n, K, 64 * w, 256, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) PsT[w * 32 * SPD_TS + tile_row(r, h) * SPD_TS + li] = acc[r];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + SPD_THREADS * q, row = e >> 5, col = e & 31;
    float dv = row == col ? 1.f : 0.f;  // the pad: identity
    if (cj + row < n && cj + col < n) {
      dv = 0.f;  // the strict upper triangle of the input is never read
      if (col <= row) dv = A[(size_t)(cj + row) * lda + cj + col] - spd_sum4(PsD, row * SPD_TS + col);
    }
    Ds[row * SPD_TS + col] = dv;
    if (!diag) {
      float tv = 0.f;  // a block column left of another is whole: only rows can be pad
      if (ci + row < n) tv = A[(size_t)(ci + row) * lda + cj + col] - spd_sum4(PsT, row * SPD_TS + col);
      Ts[row * SPD_TS + col] = tv;
    }
  }
  __syncthreads();
  if (w == 0) {
    const int bad = spd_chol32(Ds, lane);
    if (lane == 0) s_bad = bad;
  }
  __syncthreads();
  if (diag) {
    if (!finish && tid == 0) {
      const int bad = s_bad;
      if (j == 0 && !keep) *info = bad != 0 ? base + bad : 0;
      else if (bad != 0 && *info == 0) *info = base + cj + bad;
    }
    if (!finish && j != nb - 1) return;  // written by the next launch (workgroup-uniform)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + SPD_THREADS * q, row = e >> 5, col = e & 31;
      if (cj + row < n && cj + col < n)
        L[(size_t)(cj + row) * ldl + cj + col] = col <= row ? Ds[row * SPD_TS + col] : Ds[col * SPD_TS + row];
    }
    return;
  }
  if (w == 0) {
    float t[SPD_B];
#pragma unroll
    for (int c = 0; c < SPD_B; ++c) t[c] = Ts[li * SPD_TS + c];
    spd_subst32<false>(t, Ds, lane);
    if (lane < 32) {
#pragma unroll
      for (int c = 0; c < SPD_B; ++c) Ts[li * SPD_TS + c] = t[c];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + SPD_THREADS * q, a = e >> 5, b = e & 31;
    if (ci + a < n) L[(size_t)(ci + a) * ldl + cj + b] = Ts[a * SPD_TS + b];  // L_ij
    if (ci + b < n) L[(size_t)(cj + a) * ldl + ci + b] = Ts[b * SPD_TS + a];  // its transpose, tile (j, i)
  }
}

// ------------------------------------------------------------------------------------------------- solve
// LDS: Ys [32][n + 4] | Ps [4][32][33] | Ts [32][33] | Ls [32][33]
template <bool BACK>
__global__ __launch_bounds__(SPD_THREADS) void spd_solve_kernel(const float* L, int ldl, int n, const float* R, int ldr, float* X,
                                                                int ldx, int nrhs, float alpha) {
  extern __shared__ __attribute__((aligned(16))) float spd_smem[];
  const int ys = n + SPD_YPAD;
  float* Ys = spd_smem;
  float* Ps = Ys + 32 * ys;
  float* Ts = Ps + 4 * 32 * SPD_TS;
  float* Ls = Ts + 32 * SPD_TS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int r0 = blockIdx.x * 32, nb = (n + SPD_B - 1) / SPD_B, q4 = n >> 2;
  for (int e = tid; e < 32 * q4; e += SPD_THREADS) {
    const int row = e / q4, c = 4 * (e - row * q4);
    f32x4 v;
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (r0 + row < nrhs) v = *reinterpret_cast<const f32x4*>(R + (size_t)(r0 + row) * ldr + c);
    *reinterpret_cast<f32x4*>(Ys + row * ys + c) = v;
  }
  __syncthreads();
  for (int step = 0; step < nb; ++step) {
    const int jb = BACK ? nb - 1 - step : step, c0 = SPD_B * jb;
    const int k0 = BACK ? c0 + SPD_B : 0, kd = BACK ? n - k0 : c0;  // the columns already solved: [k0, k0 + kd)
    {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      if (kd > 0) acc = tile_dots_ld(Ys + k0, ys, 0, 32, L + k0, ldl, c0, n, kd, 64 * w, 256, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) Ps[w * 32 * SPD_TS + tile_row(r, h) * SPD_TS + li] = acc[r];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + SPD_THREADS * q, a = e >> 5, b = e & 31;
      float v = a == b ? 1.f : 0.f;
      if (c0 + a < n && c0 + b < n) v = L[(size_t)(c0 + a) * ldl + c0 + b];
      Ls[a * SPD_TS + b] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + SPD_THREADS * q, row = e >> 5, col = e & 31;
      float v = 0.f;
      if (c0 + col < n) v = Ys[row * ys + c0 + col] - spd_sum4(Ps, row * SPD_TS + col);
      Ts[row * SPD_TS + col] = v;
    }
    __syncthreads();
    if (w == 0) {
      float t[SPD_B];
#pragma unroll
      for (int c = 0; c < SPD_B; ++c) t[c] = Ts[li * SPD_TS + c];
      spd_subst32<BACK>(t, Ls, lane);
      if (lane < 32) {
#pragma unroll
        for (int c = 0; c < SPD_B; ++c)
          if (c0 + c < n) Ys[li * ys + c0 + c] = t[c];
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < 32 * q4; e += SPD_THREADS) {
    const int row = e / q4, c = 4 * (e - row * q4);
    if (r0 + row < nrhs) {
      f32x4 v = *reinterpret_cast<const f32x4*>(Ys + row * ys + c);
      if (BACK) {
#pragma unroll
        for (int x = 0; x < 4; ++x) v[x] = alpha * v[x];
      }
      *reinterpret_cast<f32x4*>(X + (size_t)(r0 + row) * ldx + c) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------- panels
// L[c0 + a, c1 + b] = L[c1 + b, c0 + a] for the `rows` x pn block below a diagonal block (pn a multiple of 32): one
// workgroup per 32 x 32 tile, transposed through LDS.
__global__ __launch_bounds__(SPD_THREADS) void spd_mirror_kernel(float* L, int ldl, int c0, int c1, int rows) {
  __shared__ float T[32 * SPD_TS];
  const int tid = threadIdx.x, i0 = 32 * (int)blockIdx.x, j0 = c0 + 32 * (int)blockIdx.y;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + SPD_THREADS * q, a = e >> 5, b = e & 31;
    if (i0 + a < rows) T[a * SPD_TS + b] = L[(size_t)(c1 + i0 + a) * ldl + j0 + b];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + SPD_THREADS * q, a = e >> 5, b = e & 31;
    if (i0 + b < rows) L[(size_t)(j0 + a) * ldl + c1 + i0 + b] = T[b * SPD_TS + a];
  }
}

// X[i, :n] *= alpha
__global__ __launch_bounds__(SPD_THREADS) void spd_scale_kernel(float* X, int ldx, int n, int nrhs, float alpha) {
  const int q4 = n >> 2;
  const size_t total = (size_t)nrhs * q4;
  for (size_t e = (size_t)blockIdx.x * SPD_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * SPD_THREADS) {
    const size_t row = e / q4;
    f32x4* p = reinterpret_cast<f32x4*>(X + row * ldx + 4 * (e - row * q4));
    f32x4 v = *p;
#pragma unroll
    for (int x = 0; x < 4; ++x) v[x] = alpha * v[x];
    *p = v;
  }
}

// ------------------------------------------------------------------------------------------------- host
typedef struct clipfs_spd_plan SpdPlan;

int spd_check_n(int n, const char* who) {
  CLIPFS_REQUIRE(n >= 4 && n <= SPD_MAX_N && n % 4 == 0, "%s: n = %d must be a multiple of 4 in [4, %d]", who, n, SPD_MAX_N);
  return CLIPFS_OK;
}

int spd_check_matrix(const void* p, int ld, int cols, const char* name, const char* ldname, const char* who) {
  CLIPFS_REQUIRE(p != nullptr, "%s: %s is NULL", who, name);
  CLIPFS_REQUIRE(aligned16(p), "%s: %s is not 16-byte aligned", who, name);
  CLIPFS_REQUIRE(ld >= cols && ld % 4 == 0, "%s: %s = %d must be a multiple of 4 and >= n = %d", who, ldname, ld, cols);
  return CLIPFS_OK;
}

size_t spd_span(int rows, int ld, int cols) { return ((size_t)(rows - 1) * ld + cols) * sizeof(float); }

bool spd_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

unsigned spd_solve_lds(int n) { return (unsigned)((32 * (n + SPD_YPAD) + 6 * 32 * SPD_TS) * sizeof(float)); }

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_spd_plan(int n, int nrhs, struct clipfs_spd_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_spd_plan: plan is NULL");
  CLIPFS_CHECK(spd_check_n(n, "clipfs_spd_plan"));
  CLIPFS_REQUIRE(nrhs >= 1 && nrhs <= SPD_MAX_RHS, "clipfs_spd_plan: nrhs = %d outside [1, %d]", nrhs, SPD_MAX_RHS);
  SpdPlan p = {};
  p.block = SPD_B;
  p.factor_launches = (n + SPD_B - 1) / SPD_B;
  p.solve_launches = 2;
  p.factor_grid = (unsigned)p.factor_launches;
  p.solve_grid = (unsigned)((nrhs + 31) / 32);
  p.threads = SPD_THREADS;
  p.factor_lds_bytes = (unsigned)((10 * 32 * SPD_TS) * sizeof(float) + sizeof(int));
  p.solve_lds_bytes = spd_solve_lds(n);
  p.lds_bytes = p.factor_lds_bytes > p.solve_lds_bytes ? p.factor_lds_bytes : p.solve_lds_bytes;
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_spd_factor(const float* A, int lda, float* L, int ldl, int n, int32_t* info, void* stream) {
  const char* who = "clipfs_spd_factor";
  CLIPFS_CHECK(spd_check_n(n, who));
  CLIPFS_CHECK(spd_check_matrix(A, lda, n, "A", "lda", who));
  CLIPFS_CHECK(spd_check_matrix(L, ldl, n, "L", "ldl", who));
  CLIPFS_REQUIRE(info != nullptr, "%s: info is NULL", who);
  CLIPFS_REQUIRE((reinterpret_cast<uintptr_t>(info) & 3u) == 0, "%s: info is not 4-byte aligned", who);
  const size_t sa = spd_span(n, lda, n), sl = spd_span(n, ldl, n);
  CLIPFS_REQUIRE((A == L && lda == ldl) || !spd_overlap(A, sa, L, sl),
                 "%s: L overlaps A (allowed only as L == A with ldl == lda)", who);
  CLIPFS_REQUIRE(!spd_overlap(info, 4, A, sa) && !spd_overlap(info, 4, L, sl), "%s: info overlaps A or L", who);
  const int nb = (n + SPD_B - 1) / SPD_B;
  for (int j = 0; j < nb; ++j)
    hipLaunchKernelGGL(spd_factor_kernel, dim3((unsigned)(nb - j + (j > 0 ? 1 : 0))), dim3(SPD_THREADS), 0, (hipStream_t)stream,
                       A, lda, L, ldl, n, j, info, 0, 0);
  return launch_status();
}

extern "C" int clipfs_spd_solve(const float* L, int ldl, int n, const float* R, int ldr, float* X, int ldx, int nrhs, float alpha,
                                void* stream) {
  const char* who = "clipfs_spd_solve";
  CLIPFS_CHECK(spd_check_n(n, who));
  CLIPFS_REQUIRE(nrhs >= 1 && nrhs <= SPD_MAX_RHS, "%s: nrhs = %d outside [1, %d]", who, nrhs, SPD_MAX_RHS);
  CLIPFS_CHECK(spd_check_matrix(L, ldl, n, "L", "ldl", who));
  CLIPFS_CHECK(spd_check_matrix(R, ldr, n, "R", "ldr", who));
  CLIPFS_CHECK(spd_check_matrix(X, ldx, n, "X", "ldx", who));
  CLIPFS_REQUIRE(isfinite(alpha), "%s: alpha = %g must be finite", who, (double)alpha);
  const size_t sl = spd_span(n, ldl, n), sr = spd_span(nrhs, ldr, n), sx = spd_span(nrhs, ldx, n);
  CLIPFS_REQUIRE((R == X && ldr == ldx) || !spd_overlap(R, sr, X, sx), "%s: X overlaps R (allowed only as X == R with ldx == ldr)",
                 who);
  CLIPFS_REQUIRE(!spd_overlap(X, sx, L, sl), "%s: X overlaps L", who);
  const unsigned lds = spd_solve_lds(n), grid = (unsigned)((nrhs + 31) / 32);
  if (lds > 64 * 1024) {  // per device, so asked for on every such call
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spd_solve_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spd_solve_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(spd_solve_kernel<false>, dim3(grid), dim3(SPD_THREADS), lds, st, L, ldl, n, R, ldr, X, ldx, nrhs, 1.f);
  hipLaunchKernelGGL(spd_solve_kernel<true>, dim3(grid), dim3(SPD_THREADS), lds, st, L, ldl, n, (const float*)X, ldx, X, ldx, nrhs,
                     alpha);
  return launch_status();
}

// ------------------------------------------------------------------------------------------------- panelled entry points
namespace clipfs {
namespace {

constexpr int SPD_PANELS_MAX_N = 16384, SPD_MIN_PANEL = 32, SPD_MAX_PANEL = 1024;
constexpr int SPD_BAND_PANELS = 4;  // rows of one trailing-update product, in panels

typedef struct clipfs_spd_panels_plan SpdPanelsPlan;

int spd_check_panels(int n, int panel, const char* who) {
  CLIPFS_REQUIRE(n >= 4 && n <= SPD_PANELS_MAX_N && n % 4 == 0, "%s: n = %d must be a multiple of 4 in [4, %d]", who, n,
                 SPD_PANELS_MAX_N);
  CLIPFS_REQUIRE(panel >= SPD_MIN_PANEL && panel <= SPD_MAX_PANEL && panel % 32 == 0,
                 "%s: panel = %d must be a multiple of 32 in [%d, %d]", who, panel, SPD_MIN_PANEL, SPD_MAX_PANEL);
  return CLIPFS_OK;
}

void spd_allow_solve_lds(unsigned lds) {
  if (lds > 64 * 1024) {  // per device, so asked for on every such call
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spd_solve_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spd_solve_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
  }
}

// C[M, N] = Res[M, N] - A[M, K] B[N, K]^T, every operand a sub-matrix view by its leading dimension; never split along K
int spd_gemm_sub(const float* A, int lda, const float* B, int ldb, const float* Res, int ldres, float* C, int ldc, int M, int N,
                 int K, void* stream) {
  clipfs_gemm_args g = {};
  g.struct_size = sizeof(g);
  g.A = A;
  g.B = B;
  g.C = C;
  g.M = M;
  g.N = N;
  g.K = K;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.alpha = -1.f;
  g.residual = Res;
  g.ldres = ldres;
  return clipfs_gemm_nt(&g, stream);
}

}  // namespace
}  // namespace clipfs

extern "C" int clipfs_spd_panels_plan(int n, int nrhs, int panel, struct clipfs_spd_panels_plan* plan) {
  const char* who = "clipfs_spd_panels_plan";
  CLIPFS_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  CLIPFS_CHECK(spd_check_panels(n, panel, who));
  CLIPFS_REQUIRE(nrhs >= 1 && nrhs <= SPD_MAX_RHS, "%s: nrhs = %d outside [1, %d]", who, nrhs, SPD_MAX_RHS);
  SpdPanelsPlan p = {};
  p.panel = panel;
  p.panels = (n + panel - 1) / panel;
  p.band = SPD_BAND_PANELS * panel;
  for (int k = 0; k < p.panels; ++k) {
    const int c0 = k * panel, pn = n - c0 < panel ? n - c0 : panel, rest = n - c0 - pn;
    p.factor_launches += (pn + SPD_B - 1) / SPD_B;
    if (rest > 0) {
      p.factor_launches += 2;  // L21 and its mirror
      p.factor_gemms += (rest + p.band - 1) / p.band;
    }
  }
  p.solve_launches = 2 * p.panels + 1;  // a substitution per panel and direction, the scaling
  p.solve_gemms = 2 * (p.panels - 1);
  p.threads = SPD_THREADS;
  const unsigned fl = (unsigned)((10 * 32 * SPD_TS) * sizeof(float) + sizeof(int));
  const unsigned sl = spd_solve_lds(n < panel ? n : panel);
  p.lds_bytes = fl > sl ? fl : sl;
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_spd_factor_panels(const float* A, int lda, float* L, int ldl, int n, int panel, int32_t* info, void* stream) {
  const char* who = "clipfs_spd_factor_panels";
  CLIPFS_CHECK(spd_check_panels(n, panel, who));
  CLIPFS_CHECK(spd_check_matrix(A, lda, n, "A", "lda", who));
  CLIPFS_CHECK(spd_check_matrix(L, ldl, n, "L", "ldl", who));
  CLIPFS_REQUIRE(info != nullptr, "%s: info is NULL", who);
  CLIPFS_REQUIRE((reinterpret_cast<uintptr_t>(info) & 3u) == 0, "%s: info is not 4-byte aligned", who);
  const size_t sa = spd_span(n, lda, n), sl = spd_span(n, ldl, n);
  CLIPFS_REQUIRE((A == L && lda == ldl) || !spd_overlap(A, sa, L, sl),
                 "%s: L overlaps A (allowed only as L == A with ldl == lda)", who);
  CLIPFS_REQUIRE(!spd_overlap(info, 4, A, sa) && !spd_overlap(info, 4, L, sl), "%s: info overlaps A or L", who);
  hipStream_t st = (hipStream_t)stream;
  const int band = SPD_BAND_PANELS * panel;
  // Panel 0 reads A; its trailing update writes the rest of the lower triangle into L, which every later panel reads.
  const float* src = A;
  int lds = lda;
  for (int c0 = 0; c0 < n; c0 += panel) {
    const int pn = n - c0 < panel ? n - c0 : panel, c1 = c0 + pn, rest = n - c1;
    const int nb = (pn + SPD_B - 1) / SPD_B;
    const float* sd = src + (size_t)c0 * lds + c0;
    float* ld = L + (size_t)c0 * ldl + c0;
    for (int j = 0; j < nb; ++j)
      hipLaunchKernelGGL(spd_factor_kernel, dim3((unsigned)(nb - j + (j > 0 ? 1 : 0))), dim3(SPD_THREADS), 0, st, sd, lds, ld, ldl,
                         pn, j, info, c0, c0 > 0 ? 1 : 0);
    if (rest > 0) {
      // L21 = A21 L11^-T: the forward substitution with the rows of A21 as right-hand sides
      const unsigned slds = spd_solve_lds(pn);
      spd_allow_solve_lds(slds);
      float* l21 = L + (size_t)c1 * ldl + c0;
      hipLaunchKernelGGL(spd_solve_kernel<false>, dim3((unsigned)((rest + 31) / 32)), dim3(SPD_THREADS), slds, st, (const float*)ld,
                         ldl, pn, src + (size_t)c1 * lds + c0, lds, l21, ldl, rest, 1.f);
      hipLaunchKernelGGL(spd_mirror_kernel, dim3((unsigned)((rest + 31) / 32), (unsigned)(pn / 32)), dim3(SPD_THREADS), 0, st, L, ldl,
                         c0, c1, rest);
      // A22 -= L21 L21^T in row bands: band b computes the columns up to its own last row only
      for (int r0 = 0; r0 < rest; r0 += band) {
        const int bh = rest - r0 < band ? rest - r0 : band;
        CLIPFS_CHECK(spd_gemm_sub(l21 + (size_t)r0 * ldl, ldl, l21, ldl, src + (size_t)(c1 + r0) * lds + c1, lds,
                                  L + (size_t)(c1 + r0) * ldl + c1, ldl, bh, r0 + bh, pn, stream));
      }
    }
    src = L;
    lds = ldl;
  }
  return launch_status();
}

extern "C" int clipfs_spd_solve_panels(const float* L, int ldl, int n, int panel, const float* R, int ldr, float* X, int ldx,
                                       int nrhs, float alpha, void* stream) {
  const char* who = "clipfs_spd_solve_panels";
  CLIPFS_CHECK(spd_check_panels(n, panel, who));
  CLIPFS_REQUIRE(nrhs >= 1 && nrhs <= SPD_MAX_RHS, "%s: nrhs = %d outside [1, %d]", who, nrhs, SPD_MAX_RHS);
  CLIPFS_CHECK(spd_check_matrix(L, ldl, n, "L", "ldl", who));
  CLIPFS_CHECK(spd_check_matrix(R, ldr, n, "R", "ldr", who));
  CLIPFS_CHECK(spd_check_matrix(X, ldx, n, "X", "ldx", who));
  CLIPFS_REQUIRE(isfinite(alpha), "%s: alpha = %g must be finite", who, (double)alpha);
  const size_t sl = spd_span(n, ldl, n), sr = spd_span(nrhs, ldr, n), sx = spd_span(nrhs, ldx, n);
  CLIPFS_REQUIRE((R == X && ldr == ldx) || !spd_overlap(R, sr, X, sx), "%s: X overlaps R (allowed only as X == R with ldx == ldr)",
                 who);
  CLIPFS_REQUIRE(!spd_overlap(X, sx, L, sl), "%s: X overlaps L", who);
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((nrhs + 31) / 32);
  spd_allow_solve_lds(spd_solve_lds(n < panel ? n : panel));
  // forward, Y L^T = R: substitute on the diagonal block, then take the panel's part out of every later column.  Panel 0
  // reads R; its update writes the later columns into X, where everything after it lives.
  const float* src = R;
  int lds = ldr;
  for (int c0 = 0; c0 < n; c0 += panel) {
    const int pn = n - c0 < panel ? n - c0 : panel, c1 = c0 + pn, rest = n - c1;
    hipLaunchKernelGGL(spd_solve_kernel<false>, dim3(grid), dim3(SPD_THREADS), spd_solve_lds(pn), st, L + (size_t)c0 * ldl + c0, ldl,
                       pn, src + c0, lds, X + c0, ldx, nrhs, 1.f);
    if (rest > 0)
      CLIPFS_CHECK(spd_gemm_sub(X + c0, ldx, L + (size_t)c1 * ldl + c0, ldl, src + c1, lds, X + c1, ldx, nrhs, rest, pn, stream));
    src = X;
    lds = ldx;
  }
  // backward, X L = Y, from the last panel: the rows of L^T are the strict upper triangle's
  const int last = (n - 1) / panel * panel;
  for (int c0 = last; c0 >= 0; c0 -= panel) {
    const int pn = n - c0 < panel ? n - c0 : panel;
    hipLaunchKernelGGL(spd_solve_kernel<true>, dim3(grid), dim3(SPD_THREADS), spd_solve_lds(pn), st, L + (size_t)c0 * ldl + c0, ldl,
                       pn, (const float*)(X + c0), ldx, X + c0, ldx, nrhs, 1.f);
    if (c0 > 0) CLIPFS_CHECK(spd_gemm_sub(X + c0, ldx, L + c0, ldl, X, ldx, X, ldx, nrhs, c0, pn, stream));
  }
  const size_t quads = (size_t)nrhs * (n >> 2);
  const unsigned sgrid = (unsigned)((quads + SPD_THREADS - 1) / SPD_THREADS < 4096 ? (quads + SPD_THREADS - 1) / SPD_THREADS : 4096);
  hipLaunchKernelGGL(spd_scale_kernel, dim3(sgrid), dim3(SPD_THREADS), 0, st, X, ldx, n, nrhs, alpha);
  return launch_status();
}
