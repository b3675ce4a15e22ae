// The adapter kernels' dispatch as data.  lora_plan() (lora.hip) is the only place that decides what an adapter call
// launches: the kernel family, the matrix-core instance, the slices of the dB / dA reductions, the layout of `work`, every
// grid and block, or a refusal with its cause.  The four entry points fill a LoraCall, plan and execute;
// clipfs_lora_plan() returns the plan without opening a GPU and tests/test_lora_plan.py pins it.
#pragma once
#include "common.h"

namespace clipfs {

typedef struct clipfs_lora_plan LoraPlan;  // clipfs.h (the C function of the same name hides the struct's in C++)

// One adapter call, as the entry points were given it.
struct LoraCall {
  const void* dy;  // [rows, nseg * segw] fp32, or its f16 image (dy_f16)
  bool dy_f16;
  const float* x;
  float* t;  // written by the down-projection, read by the backward
  const float *A, *B;
  float *dt, *dA, *dB, *dx;
  int rows, width, segw, r, nseg;
  unsigned seg_mask;
  float scale, p;
  uint64_t seed;
  uint32_t stream_base, drow0;
  uint16_t* keep_bits;  // written by the down-projection, read by the backward
  bool x_act;
  float* work;
  hipStream_t st;
};

// the aids, read once per process: CLIPFS_LORA_MFMA=0 (one-wave-per-row kernels everywhere), CLIPFS_LORA_KEEP_BITS=0
// (Philox again in the backward)
struct LoraAids {
  bool mfma, keep_bits;
};

int lora_plan(const LoraAids& aids, int op, int rows, int width, int segw, int r, int nseg, int flags, LoraPlan& p);

// the matrix-core family (lora_mfma.hip) executing a plan of family CLIPFS_LORA_FAMILY_MFMA
int lora_down_mfma(const LoraCall& c, const LoraPlan& p);
int lora_bwd_mfma(const LoraCall& c, const LoraPlan& p);

// out0[i] += scale0 * sum_slice part0[slice][i] and the same for part1 / out1, in one launch of `l` (lora.hip)
void launch_reduce_slices2(const clipfs_lora_launch& l, const float* part0, float* out0, size_t n0, int slices0, float scale0,
                           const float* part1, float* out1, size_t n1, int slices1, float scale1, hipStream_t st);

// launch `kernel` with the grid and block of the plan's launch `l`
template <typename K, typename... Args>
inline void lora_launch(K kernel, const clipfs_lora_launch& l, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(l.grid_x, l.grid_y), dim3(l.block), 0, st, args...);
}

}  // namespace clipfs
