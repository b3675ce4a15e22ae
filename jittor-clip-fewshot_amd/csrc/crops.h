// The PIL-exact crop / resize of one view, shared by csrc/crops.hip (fp32 outputs) and csrc/augmix.hip (the uint8 base
// image of an AugMix view): the record, its host validation, the kernel's re-check and the resampling of one workgroup's
// band of rows.  The arithmetic is Pillow's 8-bit path exactly as csrc/views.hip restates it (double coefficients
// normalised then quantised to 22 fractional bits, support scaled by max(in/out, 1), horizontal pass rounded to uint8
// before the vertical pass); what differs between the two users is only what is done with the three uint8 channels of a
// pixel, which the caller passes as `put(row, column, c0, c1, c2)`.
#pragma once
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

// The host validated the same table; a kernel re-checks what its reads depend on so that a device table that differs from
// it can never read outside the pool.  Uniform per view: a kernel writes nothing for a view that fails.  On success `off`,
// `W` describe the view's source.
__device__ __forceinline__ bool crop_rec_ok(const CropRec& r, const int64_t* __restrict__ src, int n_src, size_t pool_bytes,
                                            int S, int64_t& off, int64_t& W) {
  if (r.src < 0 || r.src >= n_src) return false;
  off = src[3 * r.src];
  const int64_t H = src[3 * r.src + 1];
  W = src[3 * r.src + 2];
  if (off < 0 || H <= 0 || W <= 0 || (uint64_t)(off + H * W * 3) > (uint64_t)pool_bytes) return false;
  if (r.top < 0 || r.left < 0 || r.h <= 0 || r.w <= 0 || r.top + r.h > H || r.left + r.w > W) return false;
  if (r.out_w <= 0 || r.out_h <= 0 || r.win_x < 0 || r.win_y < 0 || r.win_x + S > r.out_w || r.win_y + S > r.out_h) return false;
  return true;
}

// LDS bytes of one resampling workgroup for `kcap` taps: kx [kcap][S] | ky [kcap][CROP_ROWS] | xmin [S] | nx [S] |
// ymin [CROP_ROWS] | ny [CROP_ROWS], all ints.
inline size_t crop_lds_bytes(int S, int kcap) {
  return ((size_t)kcap * (S + CROP_ROWS) + 2 * (size_t)(S + CROP_ROWS)) * sizeof(int);
}

// One workgroup = view record `r` x the CROP_ROWS output rows from `row0`.  `put(i, ox, c0, c1, c2)` receives the uint8
// channels of output pixel (row0 + i, ox); every pixel of the band is handed over once, by one thread.
template <typename Put>
__device__ __forceinline__ void crop_band(const uint8_t* __restrict__ pool, int64_t off, int64_t W, const CropRec& r, int S,
                                          int kcap, int row0, int* crop_lds, Put put) {
  int* kx = crop_lds;
  int* ky = kx + kcap * S;
  int* xmin_s = ky + kcap * CROP_ROWS;
  int* nx_s = xmin_s + S;
  int* ymin_s = nx_s + S;
  int* ny_s = ymin_s + CROP_ROWS;
  const int rows = min(CROP_ROWS, S - row0);

  for (int c = threadIdx.x; c < S; c += blockDim.x) {
    const int xx = r.win_x + (r.flip ? S - 1 - c : c);  // the flip acts on the final S x S view
    crop_coeffs(r.filter, r.w, r.out_w, xx, kcap, kx + c, S, xmin_s[c], nx_s[c]);
  }
  for (int i = threadIdx.x; i < rows; i += blockDim.x)
    crop_coeffs(r.filter, r.h, r.out_h, r.win_y + row0 + i, kcap, ky + i, CROP_ROWS, ymin_s[i], ny_s[i]);
  __syncthreads();

  const uint8_t* img = pool + off;
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
    put(i, ox, crop_clip8(a0), crop_clip8(a1), crop_clip8(a2));
  }
}

// Host validation of the source and record tables, shared word for word by clipfs_crop_batch and clipfs_augmix_batch
// (`who` opens the message).  On success `kcap` is the batch's largest tap count.
inline int crop_check_tables(const char* who, size_t pool_bytes, const int64_t* src, int n_src, const int32_t* recs, int n,
                             int out_size, int& kcap) {
  for (int s = 0; s < n_src; ++s) {
    const int64_t off = src[3 * s], H = src[3 * s + 1], W = src[3 * s + 2];
    CLIPFS_REQUIRE(H > 0 && W > 0 && H <= CROP_MAX_SIDE && W <= CROP_MAX_SIDE,
                   "%s: source %d is %lld x %lld (each side must be in [1, %d])", who, s, (long long)H, (long long)W,
                   CROP_MAX_SIDE);
    CLIPFS_REQUIRE(off >= 0 && (uint64_t)(off + H * W * 3) <= (uint64_t)pool_bytes,
                   "%s: source %d lies outside the %zu-byte pool", who, s, pool_bytes);
  }
  kcap = 1;
  for (int v = 0; v < n; ++v) {
    const CropRec& r = reinterpret_cast<const CropRec*>(recs)[v];
    CLIPFS_REQUIRE(r.src >= 0 && r.src < n_src, "%s: view %d names source %d of %d", who, v, r.src, n_src);
    const int64_t H = src[3 * r.src + 1], W = src[3 * r.src + 2];
    CLIPFS_REQUIRE(r.top >= 0 && r.left >= 0 && r.h > 0 && r.w > 0 && r.top + r.h <= H && r.left + r.w <= W,
                   "%s: view %d box (top %d, left %d, h %d, w %d) is outside its %lld x %lld source", who, v, r.top, r.left,
                   r.h, r.w, (long long)H, (long long)W);
    CLIPFS_REQUIRE(r.flip == 0 || r.flip == 1, "%s: view %d flip %d", who, v, r.flip);
    CLIPFS_REQUIRE(r.filter == 0 || r.filter == 1, "%s: view %d filter %d", who, v, r.filter);
    CLIPFS_REQUIRE(r.out_w > 0 && r.out_h > 0 && r.win_x >= 0 && r.win_y >= 0 && r.win_x + out_size <= r.out_w &&
                       r.win_y + out_size <= r.out_h,
                   "%s: view %d window (%d, %d) + %d is outside its %d x %d resize", who, v, r.win_x, r.win_y, out_size,
                   r.out_w, r.out_h);
    const int tx = crop_taps(r.filter, r.w, r.out_w), ty = crop_taps(r.filter, r.h, r.out_h);
    CLIPFS_REQUIRE(tx <= CROP_KMAX && ty <= CROP_KMAX, "%s: view %d needs %d taps (at most %d)", who, v, tx > ty ? tx : ty,
                   CROP_KMAX);
    kcap = tx > kcap ? tx : kcap;
    kcap = ty > kcap ? ty : kcap;
  }
  return CLIPFS_OK;
}

}  // namespace clipfs
