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
#include "common.h"

namespace clipfs {

constexpr int CROP_PRECISION_BITS = 32 - 8 - 2;
constexpr int CROP_KMAX = 80;       // taps per axis the kernel supports (ceil(support) * 2 + 1)
constexpr int CROP_MAX_SIDE = 4096; // largest source side the pool accepts
constexpr int CROP_ROWS = 16;       // output rows per workgroup

struct CropRec {  // one row of the int32 [n, 12] descriptor
  int src;                  // source image index into the pool's [n_src, 3] table
  int top, left, h, w;      // crop box in the source image
  int flip;                 // horizontal flip of the final S x S view
  int out_w, out_h;         // size the crop is resized to
  int win_x, win_y;         // top-left of the S x S window taken from the resized image
  int filter;               // 0 bilinear, 1 bicubic (a = -0.5)
  int pad;
};

__host__ __device__ inline int crop_taps(int kind, int in_size, int out_size) {
  const double scale = (double)in_size / out_size;
  const double support = (kind == 0 ? 1.0 : 2.0) * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;  // Pillow's ksize: an upper bound of xmax - xmin
}

__device__ __forceinline__ double crop_filter(int kind, double x) {
  if (x < 0.0) x = -x;
  if (kind == 0) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for one output coordinate `xx` of an axis (in_size -> out_size); the
// quantised taps go to dst[0], dst[stride], ... (an LDS column).  The weights are evaluated twice (sum, then normalise)
// with the same operations, so each is the value Pillow stores.
__device__ __forceinline__ void crop_coeffs(int kind, int in_size, int out_size, int xx, int kcap, int* __restrict__ dst,
                                            int stride, int& xmin_out, int& n_out) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = (kind == 0 ? 1.0 : 2.0) * filterscale;
  const double center = 0.0 + (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > kcap) xmax = kcap;  // never taken: the host sizes kcap by the batch's largest ksize
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += crop_filter(kind, (x + xmin - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double v = crop_filter(kind, (x + xmin - center + 0.5) * ss);
    if (ww != 0.0) v /= ww;
    dst[x * stride] = v < 0 ? (int)(-0.5 + v * (1 << CROP_PRECISION_BITS)) : (int)(0.5 + v * (1 << CROP_PRECISION_BITS));
  }
  xmin_out = xmin;
  n_out = xmax;
}

__device__ __forceinline__ int crop_clip8(int v) {
  v >>= CROP_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// grid (ceil(S / CROP_ROWS), n): one workgroup = one view x CROP_ROWS output rows.  LDS (ints):
//   kx [kcap][S] | ky [kcap][CROP_ROWS] | xmin [S] | nx [S] | ymin [CROP_ROWS] | ny [CROP_ROWS]
__global__ __launch_bounds__(256) void crop_batch_kernel(const uint8_t* __restrict__ pool, size_t pool_bytes,
                                                         const int64_t* __restrict__ src, int n_src,
                                                         const CropRec* __restrict__ recs, int S, int kcap,
                                                         const float* __restrict__ mean, const float* __restrict__ stdv,
                                                         float* __restrict__ out_norm, float* __restrict__ out_raw) {
  extern __shared__ __attribute__((aligned(16))) int crop_lds[];
  int* kx = crop_lds;
  int* ky = kx + kcap * S;
  int* xmin_s = ky + kcap * CROP_ROWS;
  int* nx_s = xmin_s + S;
  int* ymin_s = nx_s + S;
  int* ny_s = ymin_s + CROP_ROWS;

  const int v = blockIdx.y;
  const int row0 = blockIdx.x * CROP_ROWS;
  const CropRec r = recs[v];
  // the host validated the same table (clipfs_crop_batch); re-check what the reads depend on so that a device table that
  // differs from it can never read outside the pool (uniform per workgroup: nothing is written for such a view)
  if (r.src < 0 || r.src >= n_src) return;
  const int64_t off = src[3 * r.src], H = src[3 * r.src + 1], W = src[3 * r.src + 2];
  if (off < 0 || H <= 0 || W <= 0 || (uint64_t)(off + H * W * 3) > (uint64_t)pool_bytes) return;
  if (r.top < 0 || r.left < 0 || r.h <= 0 || r.w <= 0 || r.top + r.h > H || r.left + r.w > W) return;
  if (r.out_w <= 0 || r.out_h <= 0 || r.win_x < 0 || r.win_y < 0 || r.win_x + S > r.out_w || r.win_y + S > r.out_h) return;
  const int rows = min(CROP_ROWS, S - row0);

  for (int c = threadIdx.x; c < S; c += blockDim.x) {
    const int xx = r.win_x + (r.flip ? S - 1 - c : c);  // the flip acts on the final S x S view
    crop_coeffs(r.filter, r.w, r.out_w, xx, kcap, kx + c, S, xmin_s[c], nx_s[c]);
  }
  for (int i = threadIdx.x; i < rows; i += blockDim.x)
    crop_coeffs(r.filter, r.h, r.out_h, r.win_y + row0 + i, kcap, ky + i, CROP_ROWS, ymin_s[i], ny_s[i]);
  __syncthreads();

  const uint8_t* img = pool + off;
  const size_t plane = (size_t)S * S;
  for (int p = threadIdx.x; p < rows * S; p += blockDim.x) {
    const int i = p / S, ox = p - i * S;
    const int nx = nx_s[ox], xmin = xmin_s[ox], ny = ny_s[i], ymin = ymin_s[i];
    int a0 = 1 << (CROP_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int yy = 0; yy < ny; ++yy) {
      const uint8_t* row = img + ((size_t)(r.top + ymin + yy) * W + (r.left + xmin)) * 3;
      int h0 = 1 << (CROP_PRECISION_BITS - 1), h1 = h0, h2 = h0;
      for (int xx = 0; xx < nx; ++xx) {
        const int k = kx[xx * S + ox];
        h0 += (int)row[3 * xx + 0] * k;
        h1 += (int)row[3 * xx + 1] * k;
        h2 += (int)row[3 * xx + 2] * k;
      }
      const int k = ky[yy * CROP_ROWS + i];
      a0 += crop_clip8(h0) * k;  // the horizontal pass is rounded to uint8 before the vertical pass (as in Pillow)
      a1 += crop_clip8(h1) * k;
      a2 += crop_clip8(h2) * k;
    }
    const float px[3] = {(float)crop_clip8(a0), (float)crop_clip8(a1), (float)crop_clip8(a2)};
    const size_t o = (size_t)v * 3 * plane + (size_t)(row0 + i) * S + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // ImageNormalize on a PIL image: (u8 - mean * 255) * ((1 / 255) / std), the formula of clipfs_tta_views
      if (out_norm) out_norm[o + c * plane] = (px[c] - mean[c] * 255.f) * ((1.f / 255.f) / stdv[c]);
      if (out_raw) out_raw[o + c * plane] = px[c] / 255.f;  // ToTensor
    }
  }
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
  for (int s = 0; s < n_src; ++s) {
    const int64_t off = src[3 * s], H = src[3 * s + 1], W = src[3 * s + 2];
    CLIPFS_REQUIRE(H > 0 && W > 0 && H <= CROP_MAX_SIDE && W <= CROP_MAX_SIDE,
                   "crop_batch: source %d is %lld x %lld (each side must be in [1, %d])", s, (long long)H, (long long)W,
                   CROP_MAX_SIDE);
    CLIPFS_REQUIRE(off >= 0 && (uint64_t)(off + H * W * 3) <= (uint64_t)pool_bytes,
                   "crop_batch: source %d lies outside the %zu-byte pool", s, pool_bytes);
  }
  int kcap = 1;
  for (int v = 0; v < n; ++v) {
    const CropRec& r = reinterpret_cast<const CropRec*>(recs)[v];
    CLIPFS_REQUIRE(r.src >= 0 && r.src < n_src, "crop_batch: view %d names source %d of %d", v, r.src, n_src);
    const int64_t H = src[3 * r.src + 1], W = src[3 * r.src + 2];
    CLIPFS_REQUIRE(r.top >= 0 && r.left >= 0 && r.h > 0 && r.w > 0 && r.top + r.h <= H && r.left + r.w <= W,
                   "crop_batch: view %d box (top %d, left %d, h %d, w %d) is outside its %lld x %lld source", v, r.top,
                   r.left, r.h, r.w, (long long)H, (long long)W);
    CLIPFS_REQUIRE(r.flip == 0 || r.flip == 1, "crop_batch: view %d flip %d", v, r.flip);
    CLIPFS_REQUIRE(r.filter == 0 || r.filter == 1, "crop_batch: view %d filter %d", v, r.filter);
    CLIPFS_REQUIRE(r.out_w > 0 && r.out_h > 0 && r.win_x >= 0 && r.win_y >= 0 && r.win_x + out_size <= r.out_w &&
                       r.win_y + out_size <= r.out_h,
                   "crop_batch: view %d window (%d, %d) + %d is outside its %d x %d resize", v, r.win_x, r.win_y, out_size,
                   r.out_w, r.out_h);
    const int tx = crop_taps(r.filter, r.w, r.out_w), ty = crop_taps(r.filter, r.h, r.out_h);
    CLIPFS_REQUIRE(tx <= CROP_KMAX && ty <= CROP_KMAX, "crop_batch: view %d needs %d taps (at most %d)", v,
                   tx > ty ? tx : ty, CROP_KMAX);
    kcap = tx > kcap ? tx : kcap;
    kcap = ty > kcap ? ty : kcap;
  }
  const size_t lds = ((size_t)kcap * (out_size + CROP_ROWS) + 2 * (size_t)(out_size + CROP_ROWS)) * sizeof(int);
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
