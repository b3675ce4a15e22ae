// Bias gradients of the tower backward: column sums of a tall-skinny fp32 matrix (rows = tokens, cols = width ... 4 width).
// y = x W^T + b has db = sum_rows dy, a LayerNorm bias has dbeta = sum_rows dy_out: every bias gradient of a CLIP block is
// the column sum of a tensor the backward writes anyway.
//
// Two passes, bitwise deterministic (no float atomics, cdna guide Guideline 12):
//   1. grid (column tiles x row chunks): each workgroup sums its chunk of rows for 256 columns (4 waves x 64 lanes x one
//      float4 each; wave w takes the rows w, w + 4, ... of the chunk, four independent accumulators in flight) and writes
//      one row of the partial slab work[chunk, cols];
//   2. one workgroup per 64 columns adds the slab's rows in a fixed order into the gradient slots.
// With a single chunk (small row counts: the compact last block, the heads) pass 1 adds into the slots itself.
// The row -> chunk -> wave -> accumulator assignment depends on (rows, cols) only, so the scalar variant (columns or
// leading dimension not a multiple of 4, unaligned base) adds in exactly the same order as the float4 one.
#include "common.h"

namespace clipfs {

struct BiasOuts {
  float* seg[3];  // gradient slot of columns [s * seg_width, (s + 1) * seg_width); NULL = frozen, skipped
};

constexpr int kTileCols = 256;     // columns per pass-1 workgroup (float4 variant) and the unit of the chunk heuristic
constexpr int kTargetGroups = 1024;  // ~4 workgroups per CU (256 CUs)
constexpr int kMinChunkRows = 32;

static int bias_chunks(int rows, int cols) {
  const int tiles = (cols + kTileCols - 1) / kTileCols;
  int chunks = (kTargetGroups + tiles - 1) / tiles;
  const int max_chunks = (rows + kMinChunkRows - 1) / kMinChunkRows;
  chunks = chunks < max_chunks ? chunks : max_chunks;
  if (chunks < 1) chunks = 1;
  const int rpc = (rows + chunks - 1) / chunks;
  return (rows + rpc - 1) / rpc;  // no empty chunk
}

__device__ __forceinline__ bool tile_live(const BiasOuts& o, int c_lo, int c_hi, int seg_width) {
  for (int s = c_lo / seg_width; s <= (c_hi - 1) / seg_width; ++s)
    if (o.seg[s]) return true;
  return false;
}

template <int V>
struct VecT;
template <>
struct VecT<4> {
  using T = float4;
};
template <>
struct VecT<1> {
  using T = float;
};

__device__ __forceinline__ void vadd(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void vadd(float& a, const float& b) { a += b; }
__device__ __forceinline__ void vzero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void vzero(float& a) { a = 0.f; }

__device__ __forceinline__ void add_out(const BiasOuts& o, int seg_width, int c, float v) {
  float* p = o.seg[c / seg_width];
  if (p) p[c % seg_width] += v;
}

// pass 1: V = 4 (float4 loads) or 1; 256 threads = 4 waves, each wave 64 * V consecutive columns
template <int V>
__global__ __launch_bounds__(256) void bias_partial_kernel(const float* __restrict__ x, size_t ldx, int rows, int cols,
                                                           int rpc, int seg_width, BiasOuts o, float* __restrict__ work) {
  using T = typename VecT<V>::T;
  constexpr int TC = 64 * V;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c_lo = blockIdx.x * TC;
  const int c_hi = min(cols, c_lo + TC);
  if (!tile_live(o, c_lo, c_hi, seg_width)) return;  // uniform over the workgroup
  const int c = c_lo + lane * V;
  const bool live = c < cols;
  const int r0 = blockIdx.y * rpc, r1 = min(rows, r0 + rpc);
  T a0, a1, a2, a3;
  vzero(a0); vzero(a1); vzero(a2); vzero(a3);
  if (live) {
    const float* p = x + c;
    int r = r0 + w;
    for (; r + 12 < r1; r += 16) {
      const T v0 = *reinterpret_cast<const T*>(p + (size_t)r * ldx);
      const T v1 = *reinterpret_cast<const T*>(p + (size_t)(r + 4) * ldx);
      const T v2 = *reinterpret_cast<const T*>(p + (size_t)(r + 8) * ldx);
      const T v3 = *reinterpret_cast<const T*>(p + (size_t)(r + 12) * ldx);
      vadd(a0, v0); vadd(a1, v1); vadd(a2, v2); vadd(a3, v3);
    }
    for (; r < r1; r += 4) vadd(a0, *reinterpret_cast<const T*>(p + (size_t)r * ldx));
  }
  vadd(a0, a1);
  vadd(a2, a3);
  vadd(a0, a2);
  __shared__ T red[3][64];
  if (w > 0) red[w - 1][lane] = a0;
  __syncthreads();
  if (w != 0 || !live) return;
  vadd(a0, red[0][lane]);
  vadd(a0, red[1][lane]);
  vadd(a0, red[2][lane]);
  const float* s = reinterpret_cast<const float*>(&a0);
  if (gridDim.y == 1) {
#pragma unroll
    for (int j = 0; j < V; ++j) add_out(o, seg_width, c + j, s[j]);
  } else {
    *reinterpret_cast<T*>(work + (size_t)blockIdx.y * cols + c) = a0;
  }
}

// pass 2: 512 threads = 8 waves over 64 columns; wave w adds the slab rows w, w + 8, ... then the waves in order 0..7
__global__ __launch_bounds__(512) void bias_finish_kernel(const float* __restrict__ work, int chunks, int cols,
                                                          int seg_width, BiasOuts o) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float a0 = 0.f, a1 = 0.f;
  if (c < cols) {
    int k = w;
    for (; k + 8 < chunks; k += 16) {
      a0 += work[(size_t)k * cols + c];
      a1 += work[(size_t)(k + 8) * cols + c];
    }
    for (; k < chunks; k += 8) a0 += work[(size_t)k * cols + c];
  }
  __shared__ float red[7][64];
  a0 += a1;
  if (w > 0) red[w - 1][lane] = a0;
  __syncthreads();
  if (w != 0 || c >= cols) return;
#pragma unroll
  for (int j = 0; j < 7; ++j) a0 += red[j][lane];
  add_out(o, seg_width, c, a0);
}

}  // namespace clipfs

using namespace clipfs;

extern "C" size_t clipfs_bias_grad_work_floats(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  const int chunks = bias_chunks(rows, cols);
  return chunks > 1 ? (size_t)chunks * cols : 0;
}

extern "C" int clipfs_bias_grad(const float* x, size_t ldx, int rows, int cols, int seg_width, float* out0, float* out1,
                                float* out2, float* work, void* stream) {
  CLIPFS_REQUIRE(x && rows > 0 && cols > 0 && ldx >= (size_t)cols, "bias_grad: bad args (rows %d cols %d ldx %zu)", rows,
                 cols, ldx);
  if (seg_width <= 0) seg_width = cols;
  CLIPFS_REQUIRE(cols <= 3 * seg_width, "bias_grad: %d columns need more than 3 segments of %d", cols, seg_width);
  BiasOuts o = {{out0, cols > seg_width ? out1 : nullptr, cols > 2 * seg_width ? out2 : nullptr}};
  if (!o.seg[0] && !o.seg[1] && !o.seg[2]) return CLIPFS_OK;  // every slot frozen: nothing to do
  const int chunks = bias_chunks(rows, cols);
  const int rpc = (rows + chunks - 1) / chunks;
  CLIPFS_REQUIRE(chunks == 1 || work, "bias_grad: work buffer required (%zu floats)",
                 clipfs_bias_grad_work_floats(rows, cols));
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (cols % 4) == 0 && (ldx % 4) == 0 && ((uintptr_t)x % 16) == 0;
  CLIPFS_REQUIRE(chunks == 1 || ((uintptr_t)work % 16) == 0, "bias_grad: work buffer must be 16-byte aligned");
  if (vec)
    hipLaunchKernelGGL(bias_partial_kernel<4>, dim3((cols + 255) / 256, chunks), dim3(256), 0, st, x, ldx, rows, cols, rpc,
                       seg_width, o, work);
  else
    hipLaunchKernelGGL(bias_partial_kernel<1>, dim3((cols + 63) / 64, chunks), dim3(256), 0, st, x, ldx, rows, cols, rpc,
                       seg_width, o, work);
  CLIPFS_CHECK(launch_status());
  if (chunks == 1) return CLIPFS_OK;
  hipLaunchKernelGGL(bias_finish_kernel, dim3((cols + 63) / 64), dim3(512), 0, st, work, chunks, cols, seg_width, o);
  return launch_status();
}
