// LoRA adapter kernels.  The reference materialises B@A ([d,d]) and runs a second full d x d GEMM
// per adapted projection (lora_train_vlp.py:218-221,302: +26 % FLOPs); here the rank-r form is kept:
//   down : t = drop(x) A^T           [rows, nseg*r]   (this file, HBM-bound: one read of x)
//   up   : y += scale * t B^T        (fused into the GEMM epilogue, gemm.hip)
// and the backward is three skinny products that each read their big operand exactly once.
#include "lora.h"

#include <stdlib.h>

namespace clipfs {

constexpr int LORA_MAX_CHUNKS = 8;  // width <= 2048 (one-wave-per-row kernel; the matrix-core kernel has no such bound)
constexpr int LORA_MAX_WIDTH = 4096;  // c_proj's input, 4 d
constexpr int LORA_MAX_OUT = 64;    // nseg * r of the one-wave-per-row kernel (the matrix-core kernels: 3 x 64)

// one wave per row
__global__ __launch_bounds__(256) void lora_down_kernel(const float* __restrict__ x, const float* __restrict__ A,
                                                        float* __restrict__ t, int rows, int width, int r, int nseg,
                                                        unsigned seg_mask, float p, uint64_t seed,
                                                        uint32_t stream_base, uint32_t drow0) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nch = width >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * width);
  float4 v[LORA_MAX_CHUNKS];
#pragma unroll
  for (int i = 0; i < LORA_MAX_CHUNKS; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) v[i] = xr[c];
  }
  const bool drop = p > 0.f && seed != 0;
  const uint32_t thr = dropout_threshold(p);
  const float inv_keep = 1.f / (1.f - p);
  float* trow = t + (size_t)row * (nseg * r);
  for (int s = 0; s < nseg; ++s) {
    if (!((seg_mask >> s) & 1u)) {
      if (lane < r) trow[s * r + lane] = 0.f;
      continue;
    }
    float4 xs[LORA_MAX_CHUNKS];
#pragma unroll
    for (int i = 0; i < LORA_MAX_CHUNKS; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        xs[i] = v[i];
        if (drop) {
          const float4 m = dropout_scale4(seed, stream_base + s, drow0 + (uint32_t)row, (uint32_t)c, thr, inv_keep);
          xs[i].x *= m.x;
          xs[i].y *= m.y;
          xs[i].z *= m.z;
          xs[i].w *= m.w;
        }
      }
    }
    for (int j = 0; j < r; ++j) {
      const float4* ar = reinterpret_cast<const float4*>(A + (size_t)(s * r + j) * width);
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < LORA_MAX_CHUNKS; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
          const float4 a = ar[c];
          acc += (xs[i].x * a.x + xs[i].y * a.y) + (xs[i].z * a.z + xs[i].w * a.w);
        }
      }
      acc = wave_sum(acc);
      if (lane == 0) trow[s * r + j] = acc;
    }
  }
}

// dt[m, s*r+j] = scale * sum_n dy[m, s*segw+n] * B[s*segw+n, j]     one wave per row, 16-byte loads:
// a lane takes 4 consecutive n (one float4 of dy) and the 4 matching rows of B.
template <int R>
__global__ __launch_bounds__(256) void lora_dt_kernel(const float* __restrict__ dy, const float* __restrict__ B,
                                                      float* __restrict__ dt, int rows, int segw, int nseg,
                                                      unsigned seg_mask, float scale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* dr = dy + (size_t)row * nseg * segw;
  float* out = dt + (size_t)row * nseg * R;
  for (int s = 0; s < nseg; ++s) {
    if (!((seg_mask >> s) & 1u)) {
      if (lane < R) out[s * R + lane] = 0.f;
      continue;
    }
    float acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = 0.f;
    for (int n4 = lane; n4 < (segw >> 2); n4 += 64) {
      const float4 g = *reinterpret_cast<const float4*>(dr + s * segw + 4 * n4);
      const float* b = B + ((size_t)s * segw + 4 * n4) * R;
      const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[j] = fmaf(gv[e], b[e * R + j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float v = wave_sum(acc[j]);
      if (lane == 0) out[s * R + j] = scale * v;
    }
  }
}

// Column-parallel tall reduction:  part[slice][c][j] = sum_{m in slice} X[m, c] * T[m, toff(c) + j]
// thread = one column c (coalesced across lanes), T row values are wave-uniform broadcasts.
// Used for dB (X = dy, T = t) -- deterministic two stage sum (no float atomics).
template <int R>
__global__ __launch_bounds__(256) void lora_db_partial_kernel(const float* __restrict__ dy, const float* __restrict__ t,
                                                              float* __restrict__ part, int rows, int cols, int segw,
                                                              int nseg, int rows_per_slice) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int slice = blockIdx.y;
  if (c >= cols) return;
  const int s = c / segw;
  const int m0 = slice * rows_per_slice, m1 = min(rows, m0 + rows_per_slice);
  float acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.f;
  const int tw = nseg * R;
  for (int m = m0; m < m1; ++m) {
    const float g = dy[(size_t)m * cols + c];
    const float* tr = t + (size_t)m * tw + s * R;
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = fmaf(g, tr[j], acc[j]);
  }
  float* o = part + ((size_t)slice * cols + c) * R;
#pragma unroll
  for (int j = 0; j < R; ++j) o[j] = acc[j];
}

// dA partials: thread = 4 consecutive columns k of x; acc[s][j] over the slice's rows, dropout
// multipliers regenerated from the Philox stream (never stored).  One wave per (256 columns, row slice).
// XACT: x holds a pre-activation u and the adapter's input is QuickGELU(u), applied as it is loaded (the c_proj adapter:
// only u is saved, g = QuickGELU(u) is never materialised).
template <int R, int NSEG, bool XACT = false>
__global__ __launch_bounds__(64) void lora_da_partial_kernel(const float* __restrict__ x, const float* __restrict__ dt,
                                                             float* __restrict__ part, int rows, int width,
                                                             unsigned seg_mask, float p, uint64_t seed,
                                                             uint32_t stream_base, uint32_t drow0, int rows_per_slice) {
  const int c4 = blockIdx.x * 64 + threadIdx.x;  // chunk of 4 columns
  const int slice = blockIdx.y;
  if (c4 * 4 >= width) return;
  const int m0 = slice * rows_per_slice, m1 = min(rows, m0 + rows_per_slice);
  const bool drop = p > 0.f && seed != 0;
  const uint32_t thr = dropout_threshold(p);
  const float inv_keep = 1.f / (1.f - p);
  float4 acc[NSEG][R];
#pragma unroll
  for (int s = 0; s < NSEG; ++s)
#pragma unroll
    for (int j = 0; j < R; ++j) acc[s][j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
  for (int m = m0; m < m1; ++m) {
    float4 xv = *reinterpret_cast<const float4*>(x + (size_t)m * width + 4 * c4);
    if (XACT) xv = make_float4(quick_gelu(xv.x), quick_gelu(xv.y), quick_gelu(xv.z), quick_gelu(xv.w));
    const float* dr = dt + (size_t)m * (NSEG * R);
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
      if (!((seg_mask >> s) & 1u)) continue;
      float4 xs = xv;
      if (drop) {
        const float4 mk = dropout_scale4(seed, stream_base + s, drow0 + (uint32_t)m, (uint32_t)c4, thr, inv_keep);
        xs.x *= mk.x;
        xs.y *= mk.y;
        xs.z *= mk.z;
        xs.w *= mk.w;
      }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float g = dr[s * R + j];
        acc[s][j].x = fmaf(g, xs.x, acc[s][j].x);
        acc[s][j].y = fmaf(g, xs.y, acc[s][j].y);
        acc[s][j].z = fmaf(g, xs.z, acc[s][j].z);
        acc[s][j].w = fmaf(g, xs.w, acc[s][j].w);
      }
    }
  }
  // part layout [slice][s*R + j][width]
#pragma unroll
  for (int s = 0; s < NSEG; ++s)
#pragma unroll
    for (int j = 0; j < R; ++j)
      *reinterpret_cast<float4*>(part + ((size_t)slice * (NSEG * R) + s * R + j) * width + 4 * c4) = acc[s][j];
}

// out[i] += scale * sum_slice part[slice][i].  64 outputs x 16 slice groups per block; group g sums slices
// g, g+16, ... and the 16 group sums are added in a fixed order => bitwise reproducible.
__device__ __forceinline__ void reduce_slices_body(const float* __restrict__ part, float* __restrict__ out, size_t n,
                                                   int slices, float scale, unsigned block, float (*red)[64]) {
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const size_t i = (size_t)block * 64 + lane;
  float acc = 0.f;
  if (i < n)
    for (int s = grp; s < slices; s += 16) acc += part[(size_t)s * n + i];
  red[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && i < n) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += red[g][lane];
    out[i] += scale * t;
  }
}

__global__ __launch_bounds__(1024) void reduce_slices_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                             size_t n, int slices, float scale) {
  __shared__ float red[16][64];
  reduce_slices_body(part, out, n, slices, scale, blockIdx.x, red);
}

__global__ __launch_bounds__(1024) void reduce_slices2_kernel(const float* __restrict__ part0, float* __restrict__ out0,
                                                              size_t n0, int slices0, float scale0,
                                                              const float* __restrict__ part1, float* __restrict__ out1,
                                                              size_t n1, int slices1, float scale1, unsigned nblk0) {
  __shared__ float red[16][64];
  if (blockIdx.x < nblk0)
    reduce_slices_body(part0, out0, n0, slices0, scale0, blockIdx.x, red);
  else
    reduce_slices_body(part1, out1, n1, slices1, scale1, blockIdx.x - nblk0, red);
}

// dx[m,k] += sum_{s,j} dt[m, s*r+j] * A[s*r+j, k] * dropscale_s(m,k)       one wave per row
__global__ __launch_bounds__(256) void lora_dx_kernel(const float* __restrict__ dt, const float* __restrict__ A,
                                                      float* __restrict__ dx, int rows, int width, int r, int nseg,
                                                      unsigned seg_mask, float p, uint64_t seed,
                                                      uint32_t stream_base, uint32_t drow0) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nch = width >> 2;
  const bool drop = p > 0.f && seed != 0;
  const uint32_t thr = dropout_threshold(p);
  const float inv_keep = 1.f / (1.f - p);
  const float* dr = dt + (size_t)row * nseg * r;
  float4* xr = reinterpret_cast<float4*>(dx + (size_t)row * width);
  for (int c = lane; c < nch; c += 64) {
    float4 tot = xr[c];
    for (int s = 0; s < nseg; ++s) {
      if (!((seg_mask >> s) & 1u)) continue;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int j = 0; j < r; ++j) {
        const float g = dr[s * r + j];
        const float4 av = *reinterpret_cast<const float4*>(A + (size_t)(s * r + j) * width + 4 * c);
        a.x = fmaf(g, av.x, a.x);
        a.y = fmaf(g, av.y, a.y);
        a.z = fmaf(g, av.z, a.z);
        a.w = fmaf(g, av.w, a.w);
      }
      if (drop) {
        const float4 mk = dropout_scale4(seed, stream_base + s, drow0 + (uint32_t)row, (uint32_t)c, thr, inv_keep);
        a.x *= mk.x;
        a.y *= mk.y;
        a.z *= mk.z;
        a.w *= mk.w;
      }
      tot.x += a.x;
      tot.y += a.y;
      tot.z += a.z;
      tot.w += a.w;
    }
    xr[c] = tot;
  }
}

// dg[i] *= QuickGELU'(u[i]), in place: the c_proj dgrad of a block with a c_proj adapter runs without the activation in
// its epilogue (the adapter's term is added to dg first).  16-byte accesses over n4 float4s, grid-stride; the up to 3
// trailing floats go to the first threads of block 0.
__global__ __launch_bounds__(256) void gelu_bwd_inplace_kernel(float* __restrict__ dg, const float* __restrict__ u, size_t n4,
                                                               size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 g = reinterpret_cast<float4*>(dg)[i];
    const float4 uv = reinterpret_cast<const float4*>(u)[i];
    g.x *= quick_gelu_grad(uv.x);
    g.y *= quick_gelu_grad(uv.y);
    g.z *= quick_gelu_grad(uv.z);
    g.w *= quick_gelu_grad(uv.w);
    reinterpret_cast<float4*>(dg)[i] = g;
  }
  const size_t tail = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 3 && tail < n) dg[tail] *= quick_gelu_grad(u[tail]);
}

// ---- the plan ---------------------------------------------------------------------------------------------------

constexpr int MFMA = CLIPFS_LORA_FAMILY_MFMA, ROW = CLIPFS_LORA_FAMILY_ROW;
static const char* const LORA_OP_NAME[] = {"lora_down", "lora_bwd", "lora_bwd_f16dy"};

static LoraAids lora_aids() {
  static const LoraAids a = {(getenv("CLIPFS_LORA_MFMA") ? atoi(getenv("CLIPFS_LORA_MFMA")) : 1) != 0,
                             (getenv("CLIPFS_LORA_KEEP_BITS") ? atoi(getenv("CLIPFS_LORA_KEEP_BITS")) : 1) != 0};
  return a;
}

// why the matrix-core family declines a shape; nullptr: it takes it
static const char* lora_mfma_declines(const LoraAids& aids, int width, int segw, int r, int nseg) {
  if (!aids.mfma) return "switched off by CLIPFS_LORA_MFMA=0";
  if (r < 1 || r > 64) return "they take ranks 1 ... 64";
  if (nseg != 1 && nseg != 3) return "they take 1 or 3 segments";
  if (width % 128) return "they need width % 128 == 0";
  if (segw % 64) return "they need segw % 64 == 0";
  return nullptr;
}

// Rows per reduction slice of the row family: 64 for large row counts, smaller when there are few rows so that the
// partial kernels still put >= ~1000 waves on the chip (per-rank batches of 32 images: M = 1600).
static int lora_slice_rows(int rows) {
  int r = 64;
  while (r > 8 && (rows + r - 1) / r < 256) r >>= 1;
  return r;
}

// ... of the matrix-core family: enough slices to put ~6000 wave-groups (column groups x rank groups x slices) of work on
// the chip, few enough that the partial sums stay small; never below 64 rows.  A wave does all G rank groups of its
// columns, so a larger rank needs fewer slices for the same work.
static int lora_mfma_slice_rows(int rows, int col_groups) {
  int sr = 2048;
  while (sr > 64 && (long)col_groups * ((rows + sr - 1) / sr) < 6144) sr >>= 1;
  return sr;
}

static unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

static void lora_add_launch(LoraPlan& p, unsigned grid_x, unsigned grid_y, unsigned block) {
  p.launch[p.launches++] = {grid_x, grid_y, block};
}

// The backward in p.family: slices, layout of `work`, launches.  Geometry alone -- what a family takes is lora_plan's.
static void lora_bwd_geometry(LoraPlan& p, int rows, int width, int segw, int r, int nseg, int flags) {
  const bool grads = !(flags & CLIPFS_LORA_FLAG_FROZEN), dx = (flags & CLIPFS_LORA_FLAG_DX) != 0;
  const int cols = nseg * segw;
  const size_t nb = (size_t)cols * r, na = (size_t)nseg * r * width;  // dB / dA floats per slice
  if (p.family == MFMA) {
    p.groups = (r + 15) / 16;
    p.rq = r <= 16 ? (r + 3) / 4 : 4 * p.groups;  // dx: ceil(r / 4) K-steps in one rank group, whole groups of 4 above
    p.sr_b = lora_mfma_slice_rows(rows, cols / 64 * p.groups);
    p.sr_a = lora_mfma_slice_rows(rows, width / 64 * p.groups);
  } else {
    p.sr_b = p.sr_a = lora_slice_rows(rows);
  }
  // frozen adapter: no dB / dA workgroups, no slice sums (dt and dx come out bitwise the same)
  p.slices_b = grads ? (rows + p.sr_b - 1) / p.sr_b : 0;
  p.slices_a = grads ? (rows + p.sr_a - 1) / p.sr_a : 0;
  p.part_a_offset = ((size_t)p.slices_b * nb + 3) & ~(size_t)3;  // (nb is a multiple of 4 wherever segw == width)
  p.work_floats = p.part_a_offset + (size_t)p.slices_a * na;
  const unsigned rows16 = cdiv(rows, 16), rows4 = cdiv(rows, 4);
  if (p.family == MFMA) {
    // dt and dB both read dy and do not depend on each other; dA and dx both need dt and touch different tensors: each
    // pair is one launch whose leading blocks do the partials of 256 columns x one slice, the trailing ones 16 rows
    lora_add_launch(p, cdiv(cols, 256) * p.slices_b + rows16, 1, 256);
    if (grads || dx) lora_add_launch(p, cdiv(width, 256) * p.slices_a + (dx ? rows16 : 0), 1, 256);
    if (grads) lora_add_launch(p, cdiv(nb, 64) + cdiv(na, 64), 1, 1024);
  } else {
    lora_add_launch(p, rows4, 1, 256);  // dt
    if (grads) {
      lora_add_launch(p, cdiv(cols, 256), p.slices_b, 256);  // dB partials, deterministic two-stage sum
      lora_add_launch(p, cdiv(nb, 64), 1, 1024);
      lora_add_launch(p, cdiv(width / 4, 64), p.slices_a, 64);  // dA partials
      lora_add_launch(p, cdiv(na, 64), 1, 1024);
    }
    if (dx) lora_add_launch(p, rows4, 1, 256);
  }
}

int lora_plan(const LoraAids& aids, int op, int rows, int width, int segw, int r, int nseg, int flags, LoraPlan& p) {
  CLIPFS_REQUIRE(op >= CLIPFS_LORA_OP_DOWN && op <= CLIPFS_LORA_OP_BWD_F16DY, "lora_plan: operation %d unknown", op);
  const char* who = LORA_OP_NAME[op];
  const bool keep = (flags & CLIPFS_LORA_FLAG_KEEP_BITS) != 0, x_act = (flags & CLIPFS_LORA_FLAG_X_ACT) != 0;
  if (op == CLIPFS_LORA_OP_DOWN) {
    segw = width;
    CLIPFS_REQUIRE(rows > 0 && width > 0 && (width & 3) == 0 && width <= LORA_MAX_WIDTH,
                   "%s: rows %d width %d unsupported (width a multiple of 4 up to %d)", who, rows, width, LORA_MAX_WIDTH);
  } else {
    CLIPFS_REQUIRE(nseg == 1 || nseg == 3, "%s: nseg %d unsupported (1 or 3)", who, nseg);
    // segw != width: one segment whose output width differs from its input width (the MLP linears: d -> 4d, 4d -> d)
    CLIPFS_REQUIRE(rows > 0 && width > 0 && (width & 3) == 0 && (segw == width || (nseg == 1 && segw > 0 && (segw & 3) == 0)),
                   "%s: rows %d width %d segw %d nseg %d unsupported (segw must equal width unless nseg is 1; both multiples of 4)",
                   who, rows, width, segw, nseg);
    CLIPFS_REQUIRE(!x_act || (op == CLIPFS_LORA_OP_BWD && nseg == 1 && !keep), "%s: x_act needs nseg 1, no keep bits and an fp32 dy", who);
  }
  const char* why = lora_mfma_declines(aids, width, segw, r, nseg);
  p = LoraPlan{};
  p.family = why ? ROW : MFMA;
  p.f16dy_ok = !why && segw == width;
  p.keep_bits_ok = p.f16dy_ok && aids.keep_bits;
  CLIPFS_REQUIRE(!keep || p.keep_bits_ok, "%s: keep bits are %s by the matrix-core kernels only, where segw equals width (width %d segw %d r %d nseg %d: %s)",
                 who, op == CLIPFS_LORA_OP_DOWN ? "recorded" : "read", width, segw, r, nseg,
                 why ? why : segw != width ? "segw differs" : "switched off by CLIPFS_LORA_KEEP_BITS=0");
  CLIPFS_REQUIRE(op != CLIPFS_LORA_OP_BWD_F16DY || p.f16dy_ok, "%s: width %d segw %d r %d nseg %d is outside the matrix-core kernels (%s)",
                 who, width, segw, r, nseg, why ? why : "segw differs from width");
  if (op == CLIPFS_LORA_OP_DOWN) {
    // widths above 2048 (the c_proj adapter's input) and more than 64 outputs per row run on the matrix-core kernel only
    CLIPFS_REQUIRE(!why || width <= 256 * LORA_MAX_CHUNKS, "%s: width %d needs the matrix-core kernels: %s", who, width, why);
    CLIPFS_REQUIRE(!why || (r > 0 && nseg > 0 && nseg <= 4 && nseg * r <= LORA_MAX_OUT),
                   "%s: rank %d x %d segments unsupported at width %d (%d outputs per row at most off the matrix-core kernels: %s)",
                   who, r, nseg, width, LORA_MAX_OUT, why);
    p.groups = why ? 0 : (r + 15) / 16;
    lora_add_launch(p, why ? cdiv(rows, 4) : cdiv(rows, 16), 1, 256);
    return CLIPFS_OK;
  }
  CLIPFS_REQUIRE(!why || r == 1 || r == 2 || r == 4 || r == 8 || r == 16,
                 "%s: rank %d unsupported at width %d segw %d (one-wave-per-row kernels: 1, 2, 4, 8, 16; matrix-core kernels: %s)",
                 who, r, width, segw, why);
  lora_bwd_geometry(p, rows, width, segw, r, nseg, flags);
  return CLIPFS_OK;
}

void launch_reduce_slices2(const clipfs_lora_launch& l, const float* part0, float* out0, size_t n0, int slices0, float scale0,
                           const float* part1, float* out1, size_t n1, int slices1, float scale1, hipStream_t st) {
  hipLaunchKernelGGL(reduce_slices2_kernel, dim3(l.grid_x), dim3(l.block), 0, st, part0, out0, n0, slices0, scale0, part1, out1,
                     n1, slices1, scale1, cdiv(n0, 64));  // blocks [0, ceil(n0 / 64)) take the first
}

// ---- the row family executing a plan ------------------------------------------------------------------------------

template <int R>
static int lora_bwd_row(const LoraCall& c, const LoraPlan& p) {
  const float* dy = static_cast<const float*>(c.dy);
  const int cols = c.nseg * c.segw;
  const clipfs_lora_launch* l = p.launch;
  lora_launch(lora_dt_kernel<R>, *l++, c.st, dy, c.B, c.dt, c.rows, c.segw, c.nseg, c.seg_mask, c.scale);
  CLIPFS_CHECK(launch_status());
  if (c.dA) {  // dA == dB == NULL: frozen adapter, dt and dx only
    lora_launch(lora_db_partial_kernel<R>, *l++, c.st, dy, c.t, c.work, c.rows, cols, c.segw, c.nseg, p.sr_b);
    CLIPFS_CHECK(launch_status());
    lora_launch(reduce_slices_kernel, *l++, c.st, c.work, c.dB, (size_t)cols * R, p.slices_b, c.scale);
    CLIPFS_CHECK(launch_status());
    float* part_a = c.work + p.part_a_offset;
    const auto da = c.nseg == 3 ? lora_da_partial_kernel<R, 3, false>
                                : c.x_act ? lora_da_partial_kernel<R, 1, true> : lora_da_partial_kernel<R, 1, false>;
    lora_launch(da, *l++, c.st, c.x, c.dt, part_a, c.rows, c.width, c.seg_mask, c.p, c.seed, c.stream_base, c.drow0, p.sr_a);
    CLIPFS_CHECK(launch_status());
    lora_launch(reduce_slices_kernel, *l++, c.st, part_a, c.dA, (size_t)c.nseg * R * c.width, p.slices_a, 1.0f);
    CLIPFS_CHECK(launch_status());
  }
  if (c.dx) {
    lora_launch(lora_dx_kernel, *l++, c.st, c.dt, c.A, c.dx, c.rows, c.width, R, c.nseg, c.seg_mask, c.p, c.seed, c.stream_base,
                c.drow0);
    CLIPFS_CHECK(launch_status());
  }
  return CLIPFS_OK;
}

// the three backward entry points: validate, plan, execute
static int lora_bwd(int op, const LoraCall& c) {
  const char* who = LORA_OP_NAME[op];
  CLIPFS_REQUIRE((c.dA == nullptr) == (c.dB == nullptr), "%s: dA and dB must both be given or both NULL (frozen adapter)", who);
  CLIPFS_REQUIRE(c.dy && c.x && c.t && c.A && c.B && c.dt && c.work, "%s: null pointer", who);
  CLIPFS_REQUIRE(c.p >= 0.f && c.p < 1.f, "%s: dropout p out of range", who);
  // (dy as well: every kernel of both families reads it 16 bytes at a time)
  CLIPFS_REQUIRE(aligned16(c.dy) && aligned16(c.x) && aligned16(c.A) && aligned16(c.work) && (!c.dx || aligned16(c.dx)),
                 "%s: misaligned pointer", who);
  LoraPlan p;
  CLIPFS_CHECK(lora_plan(lora_aids(), op, c.rows, c.width, c.segw, c.r, c.nseg,
                         (c.x_act ? CLIPFS_LORA_FLAG_X_ACT : 0) | (c.keep_bits ? CLIPFS_LORA_FLAG_KEEP_BITS : 0) |
                             (c.dA ? 0 : CLIPFS_LORA_FLAG_FROZEN) | (c.dx ? CLIPFS_LORA_FLAG_DX : 0), p));
  if (p.family == MFMA) return lora_bwd_mfma(c, p);
  switch (c.r) {  // (the plan admits no other rank to this family)
    case 1: return lora_bwd_row<1>(c, p);
    case 2: return lora_bwd_row<2>(c, p);
    case 4: return lora_bwd_row<4>(c, p);
    case 8: return lora_bwd_row<8>(c, p);
    default: return lora_bwd_row<16>(c, p);
  }
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_lora_plan(int op, int rows, int width, int segw, int r, int nseg, int flags, struct clipfs_lora_plan* plan) {
  CLIPFS_REQUIRE(plan, "lora_plan: null plan");
  LoraPlan p;
  CLIPFS_CHECK(lora_plan(lora_aids(), op, rows, width, segw, r, nseg, flags, p));
  *plan = p;
  return CLIPFS_OK;
}

// whether the forward can record its dropout masks as keep bits for the backward / the backward can read dy as f16
extern "C" int clipfs_lora_keep_bits_ok(int width, int segw, int r, int nseg) {
  LoraPlan p;
  return lora_plan(lora_aids(), CLIPFS_LORA_OP_BWD, 1, width, segw, r, nseg, 0, p) == CLIPFS_OK && p.keep_bits_ok;
}

extern "C" int clipfs_lora_bwd_f16dy_ok(int width, int segw, int r, int nseg) {
  LoraPlan p;
  return lora_plan(lora_aids(), CLIPFS_LORA_OP_BWD, 1, width, segw, r, nseg, 0, p) == CLIPFS_OK && p.f16dy_ok;
}

extern "C" int clipfs_lora_down(const float* x, const float* A, float* t, int rows, int width, int r, int nseg,
                                unsigned seg_mask, float p, uint64_t seed, uint32_t stream_base, uint32_t drow0, void* keep_bits,
                                void* stream) {
  const LoraCall c = {.x = x, .t = t, .A = A, .rows = rows, .width = width, .segw = width, .r = r, .nseg = nseg,
                      .seg_mask = seg_mask, .p = p, .seed = seed, .stream_base = stream_base, .drow0 = drow0,
                      .keep_bits = static_cast<uint16_t*>(keep_bits), .st = (hipStream_t)stream};
  CLIPFS_REQUIRE(x && A && t, "lora_down: null pointer");
  CLIPFS_REQUIRE(p >= 0.f && p < 1.f, "lora_down: dropout p %f out of range", (double)p);
  CLIPFS_REQUIRE(aligned16(x) && aligned16(A), "lora_down: misaligned pointer");
  LoraPlan pl;
  CLIPFS_CHECK(lora_plan(lora_aids(), CLIPFS_LORA_OP_DOWN, rows, width, width, r, nseg, keep_bits ? CLIPFS_LORA_FLAG_KEEP_BITS : 0, pl));
  if (pl.family == MFMA) return lora_down_mfma(c, pl);
  lora_launch(lora_down_kernel, pl.launch[0], c.st, x, A, t, rows, width, r, nseg, seg_mask, p, seed, stream_base, drow0);
  return launch_status();
}

// The work bound of a backward, whichever family takes it: r > 16 is the matrix-core family's alone; up to 16 either may
// run (CLIPFS_LORA_MFMA) and the row family, whose slices are never the longer ones, needs the most.  segw != width: an
// adapter whose output width differs from its input width (nseg == 1: the MLP linears).
extern "C" size_t clipfs_lora_bwd_work_floats2(int rows, int width, int segw, int r, int nseg) {
  if (segw != width && (rows <= 0 || width <= 0 || segw <= 0 || r <= 0 || nseg != 1)) return 0;
  if (segw != width && r > 16 && lora_mfma_declines({true, true}, width, segw, r, nseg)) return 64;  // no family: nothing to size
  LoraPlan p{};
  p.family = r > 16 ? MFMA : ROW;
  lora_bwd_geometry(p, rows, width, segw, r, nseg, 0);
  return p.work_floats + 64;
}

extern "C" size_t clipfs_lora_bwd_work_floats(int rows, int width, int r, int nseg) {
  return clipfs_lora_bwd_work_floats2(rows, width, width, r, nseg);
}

extern "C" int clipfs_lora_bwd(const float* dy, const float* x, const float* t, const float* A, const float* B,
                               float* dt, float* dA, float* dB, float* dx, int rows, int width, int segw, int r,
                               int nseg, unsigned seg_mask, float scale, float p, uint64_t seed, uint32_t stream_base, uint32_t drow0,
                               const void* keep_bits, float* work, void* stream) {
  return lora_bwd(CLIPFS_LORA_OP_BWD,
                  {.dy = dy, .x = x, .t = const_cast<float*>(t), .A = A, .B = B, .dt = dt, .dA = dA, .dB = dB, .dx = dx,
                   .rows = rows, .width = width, .segw = segw, .r = r, .nseg = nseg, .seg_mask = seg_mask, .scale = scale,
                   .p = p, .seed = seed, .stream_base = stream_base, .drow0 = drow0,
                   .keep_bits = static_cast<uint16_t*>(const_cast<void*>(keep_bits)), .work = work, .st = (hipStream_t)stream});
}

// One-segment adapter backward with a switch on how x is read: x_act == 1 means x holds the pre-activation u and the
// adapter's input was QuickGELU(u) -- applied as x is loaded for dA, so the activation is never materialised (the c_proj
// adapter: the forward saves u alone).  dx then receives the gradient wrt QuickGELU(u), not wrt u.  x_act == 0 is
// clipfs_lora_bwd with nseg 1 and no keep bits.
extern "C" int clipfs_lora_bwd_xact(const float* dy, const float* x, const float* t, const float* A, const float* B, float* dt,
                                    float* dA, float* dB, float* dx, int rows, int width, int segw, int r, float scale, float p,
                                    uint64_t seed, uint32_t stream_base, uint32_t drow0, int x_act, float* work, void* stream) {
  CLIPFS_REQUIRE(x_act == 0 || x_act == 1, "lora_bwd_xact: x_act %d (0 or 1)", x_act);
  return lora_bwd(CLIPFS_LORA_OP_BWD,
                  {.dy = dy, .x = x, .t = const_cast<float*>(t), .A = A, .B = B, .dt = dt, .dA = dA, .dB = dB, .dx = dx,
                   .rows = rows, .width = width, .segw = segw, .r = r, .nseg = 1, .seg_mask = 1u, .scale = scale, .p = p,
                   .seed = seed, .stream_base = stream_base, .drow0 = drow0, .x_act = x_act != 0, .work = work,
                   .st = (hipStream_t)stream});
}

// fp16 storage mode: the incoming gradient dy is read from its f16 image (what the dgrad GEMM consumes anyway) -- half
// the bytes of the two passes over dy, and the producer (clipfs_attention_f16_bwd) no longer has to write the fp32
// tensor at all.  Matrix-core kernels only: clipfs_lora_bwd_f16dy_ok says whether a shape is covered.
extern "C" int clipfs_lora_bwd_f16dy(const void* dy16, const float* x, const float* t, const float* A, const float* B,
                                     float* dt, float* dA, float* dB, float* dx, int rows, int width, int segw, int r,
                                     int nseg, unsigned seg_mask, float scale, float p, uint64_t seed, uint32_t stream_base,
                                     uint32_t drow0, const void* keep_bits, float* work, void* stream) {
  return lora_bwd(CLIPFS_LORA_OP_BWD_F16DY,
                  {.dy = dy16, .dy_f16 = true, .x = x, .t = const_cast<float*>(t), .A = A, .B = B, .dt = dt, .dA = dA, .dB = dB,
                   .dx = dx, .rows = rows, .width = width, .segw = segw, .r = r, .nseg = nseg, .seg_mask = seg_mask,
                   .scale = scale, .p = p, .seed = seed, .stream_base = stream_base, .drow0 = drow0,
                   .keep_bits = static_cast<uint16_t*>(const_cast<void*>(keep_bits)), .work = work, .st = (hipStream_t)stream});
}

extern "C" int clipfs_gelu_bwd_inplace(float* dg, const float* u, size_t n, void* stream) {
  CLIPFS_REQUIRE(dg && u && n > 0 && aligned16(dg) && aligned16(u), "gelu_bwd_inplace: null or misaligned pointer, or n = 0");
  const size_t n4 = n / 4;
  const size_t want = (n4 + 255) / 256;
  const unsigned blocks = (unsigned)(want > 8192 ? 8192 : (want ? want : 1));
  hipLaunchKernelGGL(gelu_bwd_inplace_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dg, u, n4, n);
  return launch_status();
}
