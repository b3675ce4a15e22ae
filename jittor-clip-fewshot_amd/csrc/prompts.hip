// Deep prompts (IVLP vision_depth / language_depth, reference jclip/model1.py:95-116): at the input of a prompted block,
// n rows of every sequence are replaced by the block's learnable prompt [n, width].
//   put:     x[row(c, j), :] = prompt[j, :]
//   harvest: g[j, :] += sum_c dx[row(c, j), :], then those rows of dx (and of its f16 image) are zeroed -- a replaced
//            row does not depend on the previous block, so no gradient flows there.
// Rows: dense (off == NULL) row(c, j) = c * seq + first + j, skipped when first + j >= seq (a trimmed text tower);
//       packed (off = off[0 .. batch] of the live-row plan) row(c, j) = off[c] + first + j, skipped past the caption's EOT.
// Both are memory-bound and tiny (batch * n * width floats per block).  The harvest sums in a fixed order with no float
// atomics (cdna guide Guideline 12): workgroup = one prompt row x 64 columns, wave w adds the sequences w, w + 16, ...
// in four accumulators (sequence w + 16 i feeds accumulator i % 4), then the 16 wave partials are added in wave order.
#include "common.h"

#include <hip/hip_fp16.h>

namespace clipfs {

constexpr int kHarvestWaves = 16;

__device__ __forceinline__ bool prompt_row(const int32_t* off, int c, int seq, int p, size_t* row) {
  if (off) {
    const int o = off[c];
    if (p >= off[c + 1] - o) return false;
    *row = (size_t)o + p;
  } else {
    if (p >= seq) return false;
    *row = (size_t)c * seq + p;
  }
  return true;
}

// grid (n, batch), 256 threads over the row's columns
__global__ __launch_bounds__(256) void prompt_put_kernel(const float* __restrict__ prompt, float* __restrict__ x,
                                                         const int32_t* __restrict__ off, int seq, int first, int width) {
  const int j = blockIdx.x, c = blockIdx.y;
  size_t row;
  if (!prompt_row(off, c, seq, first + j, &row)) return;  // uniform over the workgroup
  const float* src = prompt + (size_t)j * width;
  float* dst = x + row * width;
  for (int k = threadIdx.x; k < width; k += blockDim.x) dst[k] = src[k];
}

// grid (width / 64 rounded up, n), 1024 threads = 16 waves; lane = column
__global__ __launch_bounds__(1024) void prompt_harvest_kernel(float* __restrict__ dx, __half* __restrict__ dx16,
                                                              const int32_t* __restrict__ off, int batch, int seq,
                                                              int first, int width, float* __restrict__ g) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = blockIdx.y;
  const int col = blockIdx.x * 64 + lane;
  const bool live = col < width;
  const int p = first + j;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    for (int c0 = w; c0 < batch; c0 += 4 * kHarvestWaves) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // sequence c0 + 16 k goes to accumulator k
        const int c = c0 + k * kHarvestWaves;
        size_t row;
        if (c >= batch || !prompt_row(off, c, seq, p, &row)) continue;
        const size_t e = row * width + col;
        a[k] += dx[e];
        dx[e] = 0.f;
        if (dx16) dx16[e] = __float2half(0.f);
      }
    }
  }
  __shared__ float red[kHarvestWaves - 1][64];
  const float s = (a[0] + a[1]) + (a[2] + a[3]);
  if (w > 0) red[w - 1][lane] = s;
  __syncthreads();
  if (w != 0 || !live || !g) return;
  float t = s;
#pragma unroll
  for (int i = 0; i < kHarvestWaves - 1; ++i) t += red[i][lane];
  g[(size_t)j * width + col] += t;
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_prompt_put(const float* prompt, float* x, const int32_t* off, int batch, int seq, int first, int n,
                                 int width, void* stream) {
  CLIPFS_REQUIRE(prompt && x && batch > 0 && seq > 0 && first >= 0 && n > 0 && width > 0,
                 "prompt_put: bad args (batch %d seq %d first %d n %d width %d)", batch, seq, first, n, width);
  hipLaunchKernelGGL(prompt_put_kernel, dim3(n, batch), dim3(256), 0, (hipStream_t)stream, prompt, x, off, seq, first,
                     width);
  return launch_status();
}

extern "C" int clipfs_prompt_harvest(float* dx, void* dx16, const int32_t* off, int batch, int seq, int first, int n,
                                     int width, float* g, void* stream) {
  CLIPFS_REQUIRE(dx && batch > 0 && seq > 0 && first >= 0 && n > 0 && width > 0,
                 "prompt_harvest: bad args (batch %d seq %d first %d n %d width %d)", batch, seq, first, n, width);
  hipLaunchKernelGGL(prompt_harvest_kernel, dim3((width + 63) / 64, n), dim3(64 * kHarvestWaves), 0, (hipStream_t)stream,
                     dx, (__half*)dx16, off, batch, seq, first, width, g);
  return launch_status();
}
