// AugMix test-time views on the device (the rule: include/clipfs.h, "AUGMIX"): per view a PIL-exact crop, `width` chains
// of up to three PIL-exact image operations each, and the fp32 mix of the normalised chains with the normalised crop.
// The host samples the recipe (clipfs/augmix.py); the device does every pixel.  Three launches:
//
//   base    the crop of csrc/crops.h into base_u8 [n, S, S, 3]: grid (n, ceil(S / 16)), the resampling of
//           crop_batch_kernel with a uint8 store in place of the two fp32 ones.
//   chains  one workgroup of 1024 threads per (view, chain) with the whole S x S x 3 image resident in LDS for the chain:
//           grid (n, width).  AUTOCONTRAST / EQUALIZE: an LDS histogram (integer atomics: the counts do not depend on
//           their order), one scanning thread per channel (lo, hi, step, prefix sums), a 3 x 256 byte LUT from 768
//           threads, an in-place apply four bytes at a time.  POSTERIZE / SOLARIZE: in place, four bytes at a time, no
//           LUT.  AFFINE: reads the LDS image, writes chains_u8 (a single LDS image cannot be its own source and
//           destination), and the image is read back only if another operation follows.
//   mix     grid (n, ceil(S S / 1024)): a thread owns four consecutive pixels: 12 bytes of base_u8 and of each chain in,
//           three float4 out (one per plane).
//
// LDS LAYOUT.  The image stays byte-packed HWC, S S 3 bytes (150 528 at S = 224), the layout of base_u8 and chains_u8, so
// a load or a store of the image is a straight 16-byte copy and the point operations walk it a dword at a time (the
// channel of byte b is b mod 3).  One dword per pixel (200 704 bytes) does not fit beside nothing; three byte planes fit
// but would turn every image load and store into a 3-way byte shuffle while AFFINE, which carries the arithmetic, reads
// single bytes in either layout.  Histogram 3 KB + LUT 768 B + scan record bring a workgroup to 154 432 bytes at S = 224:
// one workgroup per CU, hence 16 waves in it.
//
// Nothing here contracts a * b + c: the library is built with -ffp-contract=off and the affine and LUT arithmetic
// spells its roundings out (__dmul_rn / __dadd_rn / __fmul_rn / __fadd_rn).
#include <math.h>

#include <cmath>

#include "crops.h"

namespace clipfs {

constexpr int AUG_MAX_S = 224, AUG_MIN_S = 8, AUG_MAX_WIDTH = 4, AUG_MAX_DEPTH = 3, AUG_MAX_N = 65536;
constexpr int AUG_THREADS = 1024;      // of the chain launch
constexpr int AUG_MIX_THREADS = 256;   // of the mix launch, four pixels each
constexpr int AUG_TAIL_BYTES = 3 * 256 * 4 + 3 * 256 + 64;  // histogram | LUT | scan record, after the image

enum { AUG_NONE = 0, AUG_AUTOCONTRAST = 1, AUG_EQUALIZE = 2, AUG_POSTERIZE = 3, AUG_SOLARIZE = 4, AUG_AFFINE = 5 };

inline size_t aug_image_bytes(int S) { return (size_t)S * S * 3; }
inline size_t aug_chain_lds(int S) { return ((aug_image_bytes(S) + 15) & ~(size_t)15) + AUG_TAIL_BYTES; }

// ------------------------------------------------------------------------------------------------------------- base
__global__ __launch_bounds__(256) void augmix_base_kernel(const uint8_t* __restrict__ pool, size_t pool_bytes,
                                                          const int64_t* __restrict__ src, int n_src,
                                                          const CropRec* __restrict__ recs, int S, int kcap,
                                                          uint8_t* __restrict__ base_u8) {
  extern __shared__ __attribute__((aligned(16))) int aug_crop_lds[];
  const int v = blockIdx.x;
  const int row0 = blockIdx.y * CROP_ROWS;
  const CropRec r = recs[v];
  int64_t off, W;
  if (!crop_rec_ok(r, src, n_src, pool_bytes, S, off, W)) return;
  uint8_t* dst = base_u8 + (size_t)v * S * S * 3;
  crop_band(pool, off, W, r, S, kcap, row0, aug_crop_lds, [&](int i, int ox, int c0, int c1, int c2) {
    uint8_t* px = dst + ((size_t)(row0 + i) * S + ox) * 3;
    px[0] = (uint8_t)c0;
    px[1] = (uint8_t)c1;
    px[2] = (uint8_t)c2;
  });
}

// ----------------------------------------------------------------------------------------------------------- chains
// A whole image between global memory and LDS.  16-byte copies when the global address allows (every view at S = 224: the
// image is 9408 x 16 bytes), single bytes otherwise (odd S, where a view starts at an odd address).
__device__ __forceinline__ void aug_load(uint8_t* img, const uint8_t* g, int nbytes) {
  if (((uintptr_t)g & 15) == 0) {
    const int nv = nbytes >> 4;
    for (int k = threadIdx.x; k < nv; k += blockDim.x) reinterpret_cast<uint4*>(img)[k] = reinterpret_cast<const uint4*>(g)[k];
    for (int b = (nv << 4) + threadIdx.x; b < nbytes; b += blockDim.x) img[b] = g[b];
  } else {
    for (int b = threadIdx.x; b < nbytes; b += blockDim.x) img[b] = g[b];
  }
}
__device__ __forceinline__ void aug_store(uint8_t* g, const uint8_t* img, int nbytes) {
  if (((uintptr_t)g & 15) == 0) {
    const int nv = nbytes >> 4;
    for (int k = threadIdx.x; k < nv; k += blockDim.x) reinterpret_cast<uint4*>(g)[k] = reinterpret_cast<const uint4*>(img)[k];
    for (int b = (nv << 4) + threadIdx.x; b < nbytes; b += blockDim.x) g[b] = img[b];
  } else {
    for (int b = threadIdx.x; b < nbytes; b += blockDim.x) g[b] = img[b];
  }
}

// ImageOps.autocontrast (cutoff 0) / ImageOps.equalize: histogram, then the LUT into lut[3][256].  Ends with a barrier.
__device__ __forceinline__ void aug_build_lut(int code, const uint8_t* img, int nbytes, unsigned* hist, uint8_t* lut,
                                              int* scan) {
  for (int k = threadIdx.x; k < 768; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  const int ndw = (nbytes + 3) >> 2;
  for (int k = threadIdx.x; k < ndw; k += blockDim.x) {
    const unsigned d = reinterpret_cast<const unsigned*>(img)[k];
    int c = (4 * k) % 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * k + j < nbytes) atomicAdd(&hist[c * 256 + ((d >> (8 * j)) & 255u)], 1u);  // the image's padding is not counted
      c = c == 2 ? 0 : c + 1;
    }
  }
  __syncthreads();
  // one thread per channel, each in a wave of its own: lo, hi, the occupied bins, and for EQUALIZE the step and the
  // running sum n before bin i in place of the count (n starts at step / 2)
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 192) {
    const int c = threadIdx.x >> 6;
    unsigned* h = hist + c * 256;
    int lo = 256, hi = -1, occupied = 0;
    unsigned total = 0, last = 0;
    for (int i = 0; i < 256; ++i) {
      const unsigned x = h[i];
      if (x) {
        if (lo == 256) lo = i;
        hi = i;
        ++occupied;
        last = x;
      }
      total += x;
    }
    const unsigned step = (total - last) / 255u;
    scan[4 * c + 0] = lo;
    scan[4 * c + 1] = hi;
    scan[4 * c + 2] = (int)step;
    scan[4 * c + 3] = occupied;
    if (code == AUG_EQUALIZE) {
      unsigned n = step / 2;
      for (int i = 0; i < 256; ++i) {
        const unsigned x = h[i];
        h[i] = n;
        n += x;
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 768; k += blockDim.x) {
    const int c = k >> 8, i = k & 255;
    const int lo = scan[4 * c], hi = scan[4 * c + 1], step = scan[4 * c + 2], occupied = scan[4 * c + 3];
    int out = i;
    if (code == AUG_AUTOCONTRAST) {
      if (hi > lo) {
        const double scale = 255.0 / (double)(hi - lo);
        const double offset = __dmul_rn(-(double)lo, scale);
        const int t = (int)__dadd_rn(__dmul_rn((double)i, scale), offset);  // int(): towards zero
        out = t < 0 ? 0 : (t > 255 ? 255 : t);
      }
    } else if (occupied > 1 && step > 0) {
      const unsigned q = hist[k] / (unsigned)step;
      out = q > 255u ? 255 : (int)q;  // the clamp of Image.point
    }
    lut[k] = (uint8_t)out;
  }
  __syncthreads();
}

// Image.transform((S, S), AFFINE, a, BILINEAR), fill 0: LDS image -> global image.
__device__ __forceinline__ void aug_affine(const uint8_t* img, uint8_t* g, int S, const double* __restrict__ a) {
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
  const double dS = (double)S;
  for (int p = threadIdx.x; p < S * S; p += blockDim.x) {
    const int y = p / S, x = p - y * S;
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    double xin = __dadd_rn(__dadd_rn(__dmul_rn(a0, xc), __dmul_rn(a1, yc)), a2);
    double yin = __dadd_rn(__dadd_rn(__dmul_rn(a3, xc), __dmul_rn(a4, yc)), a5);
    int o0 = 0, o1 = 0, o2 = 0;
    if (xin >= 0.0 && xin < dS && yin >= 0.0 && yin < dS) {  // anything else, a NaN included, is fill
      xin = __dadd_rn(xin, -0.5);
      yin = __dadd_rn(yin, -0.5);
      const double fx = floor(xin), fy = floor(yin);
      const double dx = __dadd_rn(xin, -fx), dy = __dadd_rn(yin, -fy);
      const int X = (int)fx, Y = (int)fy;  // in [-1, S - 1]
      const int x0 = min(max(X, 0), S - 1) * 3, x1 = min(max(X + 1, 0), S - 1) * 3;
      const uint8_t* r0 = img + min(max(Y, 0), S - 1) * S * 3;
      const bool two = Y + 1 >= 0 && Y + 1 < S;
      const uint8_t* r1 = img + (two ? Y + 1 : 0) * S * 3;
      int o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double p00 = (double)r0[x0 + c], p01 = (double)r0[x1 + c];
        const double v1 = __dadd_rn(p00, __dmul_rn(__dadd_rn(p01, -p00), dx));
        double v2 = v1;
        if (two) {
          const double p10 = (double)r1[x0 + c], p11 = (double)r1[x1 + c];
          v2 = __dadd_rn(p10, __dmul_rn(__dadd_rn(p11, -p10), dx));
        }
        o[c] = (int)__dadd_rn(v1, __dmul_rn(__dadd_rn(v2, -v1), dy));  // (UINT8)v: in [0, 255], towards zero
      }
      o0 = o[0], o1 = o[1], o2 = o[2];
    }
    uint8_t* q = g + (size_t)p * 3;
    q[0] = (uint8_t)o0;
    q[1] = (uint8_t)o1;
    q[2] = (uint8_t)o2;
  }
}

// grid (n, width): one workgroup = chain i of view v.  LDS: image (S S 3 bytes, padded to 16) | hist [3][256] u32 |
// lut [3][256] u8 | scan [16] int.
__global__ __launch_bounds__(AUG_THREADS) void augmix_chain_kernel(size_t pool_bytes,
                                                                   const int64_t* __restrict__ src, int n_src,
                                                                   const CropRec* __restrict__ recs, int S, int width,
                                                                   const int32_t* __restrict__ ops,
                                                                   const double* __restrict__ coef,
                                                                   const int32_t* __restrict__ depth,
                                                                   const uint8_t* base_u8, uint8_t* chains_u8) {
  extern __shared__ __attribute__((aligned(16))) uint8_t aug_lds[];
  const int v = blockIdx.x, i = blockIdx.y;
  const int nbytes = S * S * 3;
  uint8_t* img = aug_lds;
  unsigned* hist = reinterpret_cast<unsigned*>(aug_lds + ((nbytes + 15) & ~15));
  uint8_t* lut = reinterpret_cast<uint8_t*>(hist + 768);
  int* scan = reinterpret_cast<int*>(lut + 768);

  // a view whose record fails has no base image (the base launch wrote nothing): write nothing here either; a recipe the
  // host would have refused is not executed
  const CropRec r = recs[v];
  int64_t off, W;
  if (!crop_rec_ok(r, src, n_src, pool_bytes, S, off, W)) return;
  const size_t vi = (size_t)v * width + i;
  const int dep = depth[vi];
  if (dep < 0 || dep > AUG_MAX_DEPTH) return;
  int code[AUG_MAX_DEPTH], param[AUG_MAX_DEPTH];
#pragma unroll
  for (int s = 0; s < AUG_MAX_DEPTH; ++s) {
    code[s] = s < dep ? ops[(vi * 3 + s) * 2] : AUG_NONE;
    param[s] = s < dep ? ops[(vi * 3 + s) * 2 + 1] : 0;
    if (code[s] < AUG_NONE || code[s] > AUG_AFFINE) return;
    if (code[s] == AUG_POSTERIZE && (param[s] < 1 || param[s] > 8)) return;
    if (code[s] == AUG_SOLARIZE && (param[s] < 0 || param[s] > 256)) return;
  }

  const uint8_t* base = base_u8 + (size_t)v * nbytes;
  uint8_t* out = chains_u8 + vi * nbytes;
  aug_load(img, base, nbytes);
  __syncthreads();
  bool lds_valid = true;   // the LDS image is the chain's current image
  bool in_global = false;  // chains_u8[v, i] is the chain's current image
  const int ndw = (nbytes + 3) >> 2;
  unsigned* img32 = reinterpret_cast<unsigned*>(img);

#pragma unroll
  for (int s = 0; s < AUG_MAX_DEPTH; ++s) {
    const int op = code[s];  // uniform over the workgroup
    if (op == AUG_NONE) continue;
    if (!lds_valid) {
      aug_load(img, out, nbytes);
      __syncthreads();
      lds_valid = true;
    }
    if (op == AUG_AFFINE) {
      aug_affine(img, out, S, coef + (vi * 3 + s) * 6);
      __syncthreads();  // every read of the LDS image is done and the workgroup's stores are visible to all of it
      lds_valid = false;
      in_global = true;
      continue;
    }
    if (op == AUG_POSTERIZE) {
      const unsigned m8 = (~((1u << (8 - param[s])) - 1u)) & 255u, mask = m8 * 0x01010101u;
      for (int k = threadIdx.x; k < ndw; k += blockDim.x) img32[k] &= mask;
    } else if (op == AUG_SOLARIZE) {
      const unsigned thr = (unsigned)param[s];
      for (int k = threadIdx.x; k < ndw; k += blockDim.x) {
        const unsigned d = img32[k];
        unsigned o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned b = (d >> (8 * j)) & 255u;
          o |= (b < thr ? b : 255u - b) << (8 * j);
        }
        img32[k] = o;
      }
    } else {
      aug_build_lut(op, img, nbytes, hist, lut, scan);
      for (int k = threadIdx.x; k < ndw; k += blockDim.x) {
        const unsigned d = img32[k];
        unsigned o = 0;
        int c = (4 * k) % 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o |= (unsigned)lut[c * 256 + ((d >> (8 * j)) & 255u)] << (8 * j);
          c = c == 2 ? 0 : c + 1;
        }
        img32[k] = o;
      }
    }
    __syncthreads();
    in_global = false;
  }
  if (!in_global) aug_store(out, img, nbytes);
}

// -------------------------------------------------------------------------------------------------------------- mix
__device__ __forceinline__ float aug_norm(unsigned u8, float mean, float stdv) {
  // (u8 - mean * 255) * ((1 / 255) / std), the formula of crop_batch_kernel
  return __fmul_rn(__fadd_rn((float)u8, -__fmul_rn(mean, 255.f)), (1.f / 255.f) / stdv);
}

// 12 bytes = four HWC pixels from byte offset 12 q of an image; `vec` says the image starts on a 4-byte boundary
__device__ __forceinline__ void aug_read12(const uint8_t* __restrict__ im, size_t q, int npx, bool vec, unsigned px[12]) {
  const uint8_t* p = im + q * 12;
  if (vec && npx == 4) {
    const unsigned* d = reinterpret_cast<const unsigned*>(p);
    const unsigned d0 = d[0], d1 = d[1], d2 = d[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      px[j] = (d0 >> (8 * j)) & 255u;
      px[4 + j] = (d1 >> (8 * j)) & 255u;
      px[8 + j] = (d2 >> (8 * j)) & 255u;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) px[j] = j < 3 * npx ? p[j] : 0u;
  }
}

// grid (n, ceil(S S / 1024)), 256 threads, four consecutive pixels per thread
__global__ __launch_bounds__(AUG_MIX_THREADS) void augmix_mix_kernel(size_t pool_bytes, const int64_t* __restrict__ src,
                                                                     int n_src, const CropRec* __restrict__ recs, int S,
                                                                     int width, const float* __restrict__ w,
                                                                     const float* __restrict__ m,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ stdv,
                                                                     const uint8_t* __restrict__ base_u8,
                                                                     const uint8_t* __restrict__ chains_u8,
                                                                     float* __restrict__ out) {
  const int v = blockIdx.x;
  const CropRec r = recs[v];
  int64_t off, W;
  if (!crop_rec_ok(r, src, n_src, pool_bytes, S, off, W)) return;
  const int plane = S * S;
  const int q = blockIdx.y * AUG_MIX_THREADS + threadIdx.x;  // pixels 4 q .. 4 q + 3
  if (4 * q >= plane) return;
  const int npx = min(4, plane - 4 * q);
  const size_t nbytes = (size_t)plane * 3;
  const uint8_t* base = base_u8 + (size_t)v * nbytes;
  const float mv = m[v], om = __fadd_rn(1.f, -mv);
  float mu[3], sd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) mu[c] = mean[c], sd[c] = stdv[c];

  unsigned px[12];
  float tb[12], acc[12];
  aug_read12(base, q, npx, ((uintptr_t)base & 3) == 0, px);
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    tb[j] = aug_norm(px[j], mu[j % 3], sd[j % 3]);
    acc[j] = 0.f;
  }
  for (int i = 0; i < width; ++i) {
    const uint8_t* ch = chains_u8 + ((size_t)v * width + i) * nbytes;
    const float wi = w[(size_t)v * width + i];
    aug_read12(ch, q, npx, ((uintptr_t)ch & 3) == 0, px);
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(wi, aug_norm(px[j], mu[j % 3], sd[j % 3])));
  }
  float res[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) res[j] = __fadd_rn(__fmul_rn(mv, tb[j]), __fmul_rn(om, acc[j]));
  float* o = out + (size_t)v * 3 * plane + 4 * (size_t)q;
  const bool vec = npx == 4 && (plane & 3) == 0;  // out is 16-byte aligned (host-checked): every plane then is
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (vec) {
      *reinterpret_cast<float4*>(o + (size_t)c * plane) = make_float4(res[c], res[3 + c], res[6 + c], res[9 + c]);
    } else {
      for (int k = 0; k < npx; ++k) o[(size_t)c * plane + k] = res[3 * k + c];
    }
  }
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

static int augmix_plan_impl(int n, int S, int width, struct clipfs_augmix_plan* plan) {
  CLIPFS_REQUIRE(plan, "clipfs_augmix_plan: plan is NULL");
  CLIPFS_REQUIRE(n >= 1 && n <= AUG_MAX_N, "clipfs_augmix_plan: n = %d (must be in [1, %d])", n, AUG_MAX_N);
  CLIPFS_REQUIRE(S >= AUG_MIN_S && S <= AUG_MAX_S, "clipfs_augmix_plan: S = %d (must be in [%d, %d])", S, AUG_MIN_S, AUG_MAX_S);
  CLIPFS_REQUIRE(width >= 1 && width <= AUG_MAX_WIDTH, "clipfs_augmix_plan: width = %d (must be in [1, %d])", width,
                 AUG_MAX_WIDTH);
  struct clipfs_augmix_plan p = {};
  p.launches = 3;
  p.launch[CLIPFS_AUGMIX_LAUNCH_BASE] = {(unsigned)n, (unsigned)((S + CROP_ROWS - 1) / CROP_ROWS), 256u,
                                         (unsigned)crop_lds_bytes(S, CROP_KMAX)};
  p.launch[CLIPFS_AUGMIX_LAUNCH_CHAINS] = {(unsigned)n, (unsigned)width, (unsigned)AUG_THREADS, (unsigned)aug_chain_lds(S)};
  p.launch[CLIPFS_AUGMIX_LAUNCH_MIX] = {(unsigned)n, (unsigned)((S * S + 4 * AUG_MIX_THREADS - 1) / (4 * AUG_MIX_THREADS)),
                                        (unsigned)AUG_MIX_THREADS, 0u};
  p.lds_bytes = p.launch[CLIPFS_AUGMIX_LAUNCH_CHAINS].lds_bytes;
  p.base_bytes = (size_t)n * aug_image_bytes(S);
  p.chains_bytes = (size_t)n * width * aug_image_bytes(S);
  p.out_floats = (size_t)n * 3 * S * S;
  *plan = p;
  return CLIPFS_OK;
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_augmix_plan(int n, int S, int width, struct clipfs_augmix_plan* plan) {
  return augmix_plan_impl(n, S, width, plan);
}

extern "C" int clipfs_augmix_batch(const uint8_t* pool, size_t pool_bytes, const int64_t* src, const int64_t* src_dev,
                                   int n_src, const int32_t* recs, const int32_t* recs_dev, int n, int S, int width,
                                   const struct clipfs_augmix_recipe* recipe, const float* mean, const float* stdv,
                                   uint8_t* base_u8, uint8_t* chains_u8, float* out, void* stream) {
  const char* who = "clipfs_augmix_batch";
  struct clipfs_augmix_plan plan;
  CLIPFS_CHECK(augmix_plan_impl(n, S, width, &plan));
  CLIPFS_REQUIRE(recipe, "%s: recipe is NULL", who);
  CLIPFS_REQUIRE(recipe->struct_size == sizeof(struct clipfs_augmix_recipe), "%s: recipe.struct_size = %u (this library: %zu)",
                 who, recipe->struct_size, sizeof(struct clipfs_augmix_recipe));
  CLIPFS_REQUIRE(n_src > 0, "%s: n_src = %d", who, n_src);
  CLIPFS_REQUIRE(pool_bytes > 0, "%s: pool_bytes = 0", who);
  struct Ptr {
    const char* name;
    const void* p;
    unsigned align;
  };
  const Ptr ptrs[] = {{"pool", pool, 1}, {"src", src, 8}, {"src_dev", src_dev, 8}, {"recs", recs, 4}, {"recs_dev", recs_dev, 4},
                      {"ops", recipe->ops, 4}, {"ops_dev", recipe->ops_dev, 4}, {"coef", recipe->coef, 8},
                      {"coef_dev", recipe->coef_dev, 8}, {"depth", recipe->depth, 4}, {"depth_dev", recipe->depth_dev, 4},
                      {"w", recipe->w, 4}, {"w_dev", recipe->w_dev, 4}, {"m", recipe->m, 4}, {"m_dev", recipe->m_dev, 4},
                      {"mean", mean, 4}, {"std", stdv, 4}, {"base_u8", base_u8, 16}, {"chains_u8", chains_u8, 16}, {"out", out, 16}};
  for (const Ptr& q : ptrs) {
    CLIPFS_REQUIRE(q.p, "%s: %s is NULL", who, q.name);
    CLIPFS_REQUIRE((reinterpret_cast<uintptr_t>(q.p) & (q.align - 1)) == 0, "%s: %s is not %u-byte aligned", who, q.name, q.align);
  }
  const size_t out_bytes = plan.out_floats * sizeof(float);
  CLIPFS_REQUIRE(!ranges_overlap(base_u8, plan.base_bytes, chains_u8, plan.chains_bytes), "%s: chains_u8 overlaps base_u8", who);
  CLIPFS_REQUIRE(!ranges_overlap(out, out_bytes, base_u8, plan.base_bytes), "%s: out overlaps base_u8", who);
  CLIPFS_REQUIRE(!ranges_overlap(out, out_bytes, chains_u8, plan.chains_bytes), "%s: out overlaps chains_u8", who);
  CLIPFS_REQUIRE(!ranges_overlap(base_u8, plan.base_bytes, pool, pool_bytes), "%s: base_u8 overlaps pool", who);
  CLIPFS_REQUIRE(!ranges_overlap(chains_u8, plan.chains_bytes, pool, pool_bytes), "%s: chains_u8 overlaps pool", who);
  CLIPFS_REQUIRE(!ranges_overlap(out, out_bytes, pool, pool_bytes), "%s: out overlaps pool", who);

  int kcap = 1;
  CLIPFS_CHECK(crop_check_tables(who, pool_bytes, src, n_src, recs, n, S, kcap));
  const size_t base_lds = crop_lds_bytes(S, kcap);
  CLIPFS_REQUIRE(base_lds <= 160 * 1024, "%s: S %d with %d taps needs %zu bytes of LDS", who, S, kcap, base_lds);
  for (int v = 0; v < n; ++v) {
    CLIPFS_REQUIRE(std::isfinite(recipe->m[v]), "%s: m[%d] is not finite", who, v);
    for (int i = 0; i < width; ++i) {
      const size_t vi = (size_t)v * width + i;
      const int dep = recipe->depth[vi];
      CLIPFS_REQUIRE(dep >= 0 && dep <= AUG_MAX_DEPTH, "%s: depth[%d, %d] = %d (must be in [0, %d])", who, v, i, dep, AUG_MAX_DEPTH);
      CLIPFS_REQUIRE(std::isfinite(recipe->w[vi]), "%s: w[%d, %d] is not finite", who, v, i);
      for (int s = 0; s < dep; ++s) {
        const int code = recipe->ops[(vi * 3 + s) * 2], param = recipe->ops[(vi * 3 + s) * 2 + 1];
        CLIPFS_REQUIRE(code >= AUG_NONE && code <= AUG_AFFINE, "%s: ops[%d, %d, %d] code = %d (must be in [0, 5])", who, v, i, s, code);
        CLIPFS_REQUIRE(code != AUG_POSTERIZE || (param >= 1 && param <= 8), "%s: ops[%d, %d, %d] bits = %d (must be in [1, 8])", who,
                       v, i, s, param);
        CLIPFS_REQUIRE(code != AUG_SOLARIZE || (param >= 0 && param <= 256),
                       "%s: ops[%d, %d, %d] threshold = %d (must be in [0, 256])", who, v, i, s, param);
        if (code == AUG_AFFINE)
          for (int k = 0; k < 6; ++k)
            CLIPFS_REQUIRE(std::isfinite(recipe->coef[(vi * 3 + s) * 6 + k]), "%s: coef[%d, %d, %d, %d] is not finite", who, v, i, s, k);
      }
    }
  }

  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&augmix_base_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&augmix_chain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr = true;
  }
  const struct clipfs_augmix_launch &lb = plan.launch[CLIPFS_AUGMIX_LAUNCH_BASE], &lc = plan.launch[CLIPFS_AUGMIX_LAUNCH_CHAINS],
                                    &lm = plan.launch[CLIPFS_AUGMIX_LAUNCH_MIX];
  const CropRec* rd = reinterpret_cast<const CropRec*>(recs_dev);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(augmix_base_kernel, dim3(lb.grid_x, lb.grid_y), dim3(lb.block), base_lds, st, pool, pool_bytes, src_dev, n_src,
                     rd, S, kcap, base_u8);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(augmix_chain_kernel, dim3(lc.grid_x, lc.grid_y), dim3(lc.block), lc.lds_bytes, st, pool_bytes, src_dev,
                     n_src, rd, S, width, recipe->ops_dev, recipe->coef_dev, recipe->depth_dev, base_u8, chains_u8);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(augmix_mix_kernel, dim3(lm.grid_x, lm.grid_y), dim3(lm.block), 0, st, pool_bytes, src_dev, n_src, rd, S, width,
                     recipe->w_dev, recipe->m_dev, mean, stdv, base_u8, chains_u8, out);
  return launch_status();
}
