// GPU generation of few-shot TRAINING batches (the reference builds them on 8 CPU workers with PIL,
// lora_train_vlp.py:1196-1218, slow_pace.py:1903-1935):
//     RandomResizedCrop(224, scale=(0.05, 1), BILINEAR) -> RandomHorizontalFlip -> [ImageNormalize] -> ToTensor
// Every decoded training image lives once in HBM as uint8 HWC, back to back in one pool; one launch writes a whole batch
// in which each view names its own source.  The resampling is Pillow's 8-bit path exactly as csrc/views.hip restates it
// (double coefficients normalised then quantised to 22 fractional bits, support scaled by max(in/out, 1), horizontal
// pass rounded to uint8 before the vertical pass), so the pixels equal Image.crop(box).resize(...) bit for bit.
//
// Differences from views.hip: the tap count is bounded by CROP_KMAX = 80 instead of 24 (a bicubic 4096 -> 224 crop
// needs ceil(2 * 4096 / 224) * 2 + 1 = 75), and the filter coefficients are computed once per output column and once
// per output row of a workgroup's band into LDS (two passes over the taps, no per-thread array: the kernel has no
// scratch), not once per pixel.  A workgroup owns one view x CROP_ROWS output rows; the LDS tables are sized by the
// largest tap count of the batch (host-computed), so an ordinary batch uses a few KB.
#include "crops.h"  // the record, its checks and the resampling, shared with csrc/augmix.hip

namespace clipfs {

// grid (ceil(S / CROP_ROWS), n): one workgroup = one view x CROP_ROWS output rows.  LDS (ints):
//   kx [kcap][S] | ky [kcap][CROP_ROWS] | xmin [S] | nx [S] | ymin [CROP_ROWS] | ny [CROP_ROWS]
__global__ __launch_bounds__(256) void crop_batch_kernel(const uint8_t* __restrict__ pool, size_t pool_bytes,
                                                         const int64_t* __restrict__ src, int n_src,
                                                         const CropRec* __restrict__ recs, int S, int kcap,
                                                         const float* __restrict__ mean, const float* __restrict__ stdv,
                                                         float* __restrict__ out_norm, float* __restrict__ out_raw) {
  extern __shared__ __attribute__((aligned(16))) int crop_lds[];
  const int v = blockIdx.y;
  const int row0 = blockIdx.x * CROP_ROWS;
  const CropRec r = recs[v];
  int64_t off, W;
  if (!crop_rec_ok(r, src, n_src, pool_bytes, S, off, W)) return;
  const size_t plane = (size_t)S * S;
  crop_band(pool, off, W, r, S, kcap, row0, crop_lds, [&](int i, int ox, int c0, int c1, int c2) {
    const float px[3] = {(float)c0, (float)c1, (float)c2};
    const size_t o = (size_t)v * 3 * plane + (size_t)(row0 + i) * S + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // ImageNormalize on a PIL image: (u8 - mean * 255) * ((1 / 255) / std), the formula of clipfs_tta_views
      if (out_norm) out_norm[o + c * plane] = (px[c] - mean[c] * 255.f) * ((1.f / 255.f) / stdv[c]);
      if (out_raw) out_raw[o + c * plane] = px[c] / 255.f;  // ToTensor
    }
  });
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_crop_batch(const uint8_t* pool, size_t pool_bytes, const int64_t* src, const int64_t* src_dev,
                                 int n_src, const int32_t* recs, const int32_t* recs_dev, int n, int out_size,
                                 const float* mean, const float* stdv, float* out_norm, float* out_raw, void* stream) {
  CLIPFS_REQUIRE(pool && src && src_dev && recs && recs_dev, "crop_batch: null pool / source table / record table");
  CLIPFS_REQUIRE(out_norm || out_raw, "crop_batch: both outputs are NULL");
  CLIPFS_REQUIRE(!out_norm || (mean && stdv), "crop_batch: out_norm needs mean and std");
  CLIPFS_REQUIRE(n_src > 0 && n > 0 && out_size > 0 && pool_bytes > 0, "crop_batch: bad dims (n_src %d, n %d, size %d)",
                 n_src, n, out_size);
  int kcap = 1;
  CLIPFS_CHECK(crop_check_tables("crop_batch", pool_bytes, src, n_src, recs, n, out_size, kcap));
  const size_t lds = crop_lds_bytes(out_size, kcap);
  CLIPFS_REQUIRE(lds <= 160 * 1024, "crop_batch: out_size %d with %d taps needs %zu bytes of LDS", out_size, kcap, lds);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&crop_batch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(crop_batch_kernel, dim3((out_size + CROP_ROWS - 1) / CROP_ROWS, n), dim3(256), lds,
                     (hipStream_t)stream, pool, pool_bytes, src_dev, n_src, reinterpret_cast<const CropRec*>(recs_dev),
                     out_size, kcap, mean, stdv, out_norm, out_raw);
  return launch_status();
}
