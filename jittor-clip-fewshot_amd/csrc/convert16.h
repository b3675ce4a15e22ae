// fp32 -> 16-bit conversions of eight consecutive values, shared by every kernel that writes a weight's 16-bit image
// (clipfs_split_bf16 / clipfs_convert_f16 in gemm_bf16.hip, clipfs_lora_merge in lora_merge.hip), so that the images
// agree bit for bit whichever kernel wrote them.
#pragma once
#include <hip/hip_runtime.h>

namespace clipfs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// hi = bf16(x), lo = bf16(x - hi), both round to nearest even
__device__ __forceinline__ void split8(const f32x4& x0, const f32x4& x1, bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hi[j] = (__bf16)x0[j];
    hi[4 + j] = (__bf16)x1[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = (__bf16)(x0[j] - (float)hi[j]);
    lo[4 + j] = (__bf16)(x1[j] - (float)hi[4 + j]);
  }
}

__device__ __forceinline__ f16x8 to_f16x8(const f32x4& x0, const f32x4& x1) {
  f16x8 h;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = (_Float16)x0[j];
    h[4 + j] = (_Float16)x1[j];
  }
  return h;
}

}  // namespace clipfs
