// 32 x 32 fp32 tiles of row-by-row dot products on v_mfma_f32_32x32x2_f32, and the gradient walk built on them: the
// device machinery shared by cache_head.hip, tpt.hip and contrastive.hip, and later by sigmoid_pairs.hip, clip_pairs.hip,
// tda.hip, transduct.hip and spd.hip (gda.hip includes it for the shared types only).
//
// A tile is formed the way attention_mfma.hip forms its scores.  Both operands are row-major rows of d floats; the
// K-slot <-> feature assignment of an MFMA sum is free as long as A and B agree, so each half-wave takes one contiguous
// half of a step.  The product comes out with a lane holding 16 rows of the A side (tile_row) for ONE row of the B side.
// Rows past the end are clamped to the last row (the caller discards their products), features >= d read as 0; d is a
// multiple of 4, so a float4 that starts below d ends inside the row.
//
//   tile_dots         operands straight from global memory / L2: a lane reads 128 contiguous bytes of its row per
//                     64-feature step.
//   tile_dots_ld      tile_dots with a leading dimension per side (rows of a Cholesky factor, an operand in LDS): spd.hip
//   tile_dots_staged  operands through LDS in chunks of TILE_KC features, the four waves of a workgroup splitting each
//                     chunk; tile_sum4 adds their partials in wave order.
//   tile_grad_walk    out[x, :] (+)= sum_y G(x, y) Y[y, :] for one workgroup's 32 own rows and 128 NACC features, G a
//                     function of the dot product X[x, :] . Y[y, :] that the caller supplies.
//
// No float atomics: every output element is written by one thread and the order of every sum depends on the shapes alone.
#pragma once
#include "common.h"

namespace clipfs {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TILE_THREADS = 256;  // 4 waves: the workgroup of everything staged
constexpr int TILE_FEAT = 512;     // most features per gradient workgroup: 4 waves x 4 accumulators x 32
constexpr int TILE_PS = 33;        // row stride of a wave's partial tile in LDS (conflict-free transposed read)
constexpr int TILE_KC = 128, TILE_KST = TILE_KC + 4;  // + 4: 16-byte rows, conflict-free ds_read_b128 over consecutive rows
constexpr float TILE_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f32x16 tile_mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of the A side that register r of lane (half h) holds
__device__ __forceinline__ int tile_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// acc[A row a0 + tile_row(r, h)][B row b0 + (lane & 31)] = the sum over the 64-feature steps s0, s0 + sstep, ... < d:
// (0, 64) is the whole dot product, (64 w, 256) wave w's share of it.
__device__ __forceinline__ f32x16 tile_dots(const float* __restrict__ A, int a0, int na, const float* __restrict__ Bm, int b0,
                                            int nb, int d, int s0, int sstep, int lane) {
  const int li = lane & 31, h = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* pa = A + (size_t)min(a0 + li, na - 1) * d + 32 * h;
  const float* pb = Bm + (size_t)min(b0 + li, nb - 1) * d + 32 * h;
  for (int s = s0; s < d; s += sstep) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f32x4 va, vb;
      va[0] = va[1] = va[2] = va[3] = 0.f;
      vb = va;
      if (s + 32 * h + 4 * j < d) {
        va = *reinterpret_cast<const f32x4*>(pa + s + 4 * j);
        vb = *reinterpret_cast<const f32x4*>(pb + s + 4 * j);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = tile_mfma(va[e], vb[e], acc);
    }
  }
  return acc;
}

// tile_dots with a leading dimension per side (multiples of 4, rows 16-byte aligned): rows of a matrix, or of two column
// ranges of one (spd.hip: a row block of a Cholesky factor against another; the sides may be the same memory, so
// neither is __restrict__).  An operand may live in LDS.  Same clamping, same zero fill past d, same order of the sum.
__device__ __forceinline__ f32x16 tile_dots_ld(const float* A, int lda, int a0, int na, const float* Bm, int ldb, int b0, int nb,
                                               int d, int s0, int sstep, int lane) {
  const int li = lane & 31, h = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* pa = A + (size_t)min(a0 + li, na - 1) * lda + 32 * h;
  const float* pb = Bm + (size_t)min(b0 + li, nb - 1) * ldb + 32 * h;
  for (int s = s0; s < d; s += sstep) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f32x4 va, vb;
      va[0] = va[1] = va[2] = va[3] = 0.f;
      vb = va;
      if (s + 32 * h + 4 * j < d) {
        va = *reinterpret_cast<const f32x4*>(pa + s + 4 * j);
        vb = *reinterpret_cast<const f32x4*>(pb + s + 4 * j);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = tile_mfma(va[e], vb[e], acc);
    }
  }
  return acc;
}

// tile_dots' products (operands straight from global memory) summed in the ORDER of the staged tile below: per chunk of
// TILE_KC features four partial sums, the staged waves' shares of 32 features with half h taking 16 of them, added in wave
// order as tile_sum4 adds them.  A statistic made from these products (a log-sum-exp) and a gradient kernel that forms
// the products again through tile_dots_staged then hold the SAME fp32 number for every pair of rows.  With two orders the
// two differ by the rounding of a d-term fp32 sum, ~1e-7 of |a| |b|; a logit scale s multiplies that, and
// exp(s a - lse) of a row's dominant key, where s a and lse cancel, is off by s 1e-7: 1e-4 of the gradient at s = 1000.
__device__ __forceinline__ f32x16 tile_dots_as_staged(const float* __restrict__ A, int a0, int na, const float* __restrict__ Bm,
                                                      int b0, int nb, int d, int lane) {
  const int li = lane & 31, h = lane >> 5;
  f32x16 acc[4];
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[w][r] = 0.f;
  const float* pa = A + (size_t)min(a0 + li, na - 1) * d + 16 * h;
  const float* pb = Bm + (size_t)min(b0 + li, nb - 1) * d + 16 * h;
  for (int s = 0; s < d; s += TILE_KC) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (s + 32 * w < d) {  // wave-uniform; a share wholly past d is zeros in the staged tile too
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f32x4 va, vb;
          va[0] = va[1] = va[2] = va[3] = 0.f;
          vb = va;
          if (s + 32 * w + 16 * h + 4 * j < d) {
            va = *reinterpret_cast<const f32x4*>(pa + s + 32 * w + 4 * j);
            vb = *reinterpret_cast<const f32x4*>(pb + s + 32 * w + 4 * j);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[w] = tile_mfma(va[e], vb[e], acc[w]);
        }
      }
    }
  }
  f32x16 sum;
#pragma unroll
  for (int r = 0; r < 16; ++r) sum[r] = ((acc[0][r] + acc[1][r]) + acc[2][r]) + acc[3][r];
  return sum;
}

// The staged tile: 32 x 32 over the whole of d, the operands passing through LDS in chunks of TILE_KC features (16-byte
// global loads with a row's 128 features contiguous over 32 threads, where tile_dots' lanes each walk a row of their own).
// Wave w takes features [32 w, 32 w + 32) of every chunk, half h 16 of them.  The next chunk -- after a tile's last one,
// the first chunk of the tile at (a0n, b0n) -- is fetched into registers while this one is multiplied.
struct TileStage {
  f32x4 ra[4], rb[4];
  __device__ __forceinline__ void load(const float* __restrict__ A, int a0, int na, const float* __restrict__ Bm, int b0, int nb,
                                       int d, int s, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + TILE_THREADS * i, row = e >> 5, c = s + 4 * (e & 31);
      f32x4 z;
      z[0] = z[1] = z[2] = z[3] = 0.f;
      ra[i] = rb[i] = z;
      if (c < d) {
        ra[i] = *reinterpret_cast<const f32x4*>(A + (size_t)min(a0 + row, na - 1) * d + c);
        rb[i] = *reinterpret_cast<const f32x4*>(Bm + (size_t)min(b0 + row, nb - 1) * d + c);
      }
    }
  }
  __device__ __forceinline__ void store(float* sA, float* sB, int tid) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + TILE_THREADS * i, at = (e >> 5) * TILE_KST + 4 * (e & 31);
      *reinterpret_cast<f32x4*>(sA + at) = ra[i];
      *reinterpret_cast<f32x4*>(sB + at) = rb[i];
    }
  }
};
// `st` holds chunk 0 of this tile on entry and chunk 0 of the next tile (if any) on return.  The result is wave w's
// partial over its features of every chunk.  Every thread of the workgroup calls it (it synchronises).
__device__ __forceinline__ f32x16 tile_dots_staged(TileStage& st, const float* __restrict__ A, int a0, int na,
                                                   const float* __restrict__ Bm, int b0, int nb, int d, int a0n, int b0n,
                                                   bool has_next, float* sA, float* sB, int tid) {
  const int lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* pa = sA + li * TILE_KST + 32 * w + 16 * h;
  const float* pb = sB + li * TILE_KST + 32 * w + 16 * h;
  for (int s = 0; s < d; s += TILE_KC) {
    __syncthreads();  // the last chunk's reads are done
    st.store(sA, sB, tid);
    __syncthreads();
    if (s + TILE_KC < d) st.load(A, a0, na, Bm, b0, nb, d, s + TILE_KC, tid);
    else if (has_next) st.load(A, a0n, na, Bm, b0n, nb, d, 0, tid);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(pa + 4 * j);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + 4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = tile_mfma(va[e], vb[e], acc);
    }
  }
  return acc;
}

// element `at` of the four waves' partial tiles ([row][TILE_PS] records), added in wave order
__device__ __forceinline__ float tile_sum4(const float (*Ps)[32 * TILE_PS], int at) {
  return ((Ps[0][at] + Ps[1][at]) + Ps[2][at]) + Ps[3][at];
}

// The gradient kernels' body.  One workgroup of TILE_THREADS per (32 own rows of X, 128 NACC features), grid
// (ceil(NX / 32), ceil(d / (128 NACC))).  It walks Y in tiles of 32 ascending: both tiles pass through LDS (the staged
// tile, the next chunk in flight while this one is multiplied), the four waves' partials are added in wave order, G is
// formed once in LDS, then every wave contracts G with Y's rows into its 32 NACC features.  NACC: 32-feature accumulators
// per wave: 4 where the own tiles alone fill the machine, 1 (four times the workgroups, each forming the tile again)
// where they do not.  ACCUM adds to `out` instead of overwriting it.
//
// `fn` supplies what is particular to an objective:
//   fn.tile(y0, tid)           called by every thread once per tile of Y, after the partials are stored and before the
//                              barrier that precedes forming G: what it writes to LDS is visible to fn.g of this tile.
//   fn.g(a, xi, yi, own, oth)  G for the dot product a of own row xi = x0 + own < NX and other row yi = y0 + oth < NY;
//                              out-of-range elements are 0 without a call.
// `fn` is a small record of scalars and pointers, passed by value (the kernels then compile to what they were with the
// body written out in each).  Every thread of the workgroup calls the walk (it synchronises); it owns 54 784 bytes of
// LDS (tile_grad_lds_bytes).
template <bool ACCUM, int NACC, class Fn>
__device__ __forceinline__ void tile_grad_walk(const float* __restrict__ X, const float* __restrict__ Y,
                                               float* __restrict__ out, int NX, int NY, int d, Fn fn) {
  __shared__ __attribute__((aligned(16))) float sX[32 * TILE_KST];  // a chunk of the own rows
  __shared__ __attribute__((aligned(16))) float sY[32 * TILE_KST];  //   ... of the other side's tile
  __shared__ float Ps[4][32 * TILE_PS];  // per wave: [own][other] partial dot products over its features of every chunk
  __shared__ float Gs[32 * 32];          // [other][own]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * 32;
  const int fw = (blockIdx.y * 4 + w) * 32 * NACC;  // this wave's first feature
  f32x16 acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
  TileStage st;
  st.load(X, x0, NX, Y, 0, NY, d, 0, tid);
  for (int y0 = 0; y0 < NY; y0 += 32) {
    const f32x16 s = tile_dots_staged(st, X, x0, NX, Y, y0, NY, d, x0, y0 + 32, y0 + 32 < NY, sX, sY, tid);
    // the first accumulator's operands of the other side: in flight while G is formed
    float y0v[16];
    {
      const int ft = fw + li;
#pragma unroll
      for (int i = 0; i < 16; ++i) y0v[i] = ft < d ? Y[(size_t)min(y0 + 16 * h + i, NY - 1) * d + ft] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) Ps[w][tile_row(r, h) * TILE_PS + li] = s[r];
    fn.tile(y0, tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + TILE_THREADS * i, own = e & 31, oth = e >> 5;
      const float a = tile_sum4(Ps, own * TILE_PS + oth);
      const int xi = x0 + own, yi = y0 + oth;
      float g = 0.f;
      if (xi < NX && yi < NY) g = fn.g(a, xi, yi, own, oth);
      Gs[oth * 32 + own] = g;
    }
    __syncthreads();
    float ga[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) ga[i] = Gs[(16 * h + i) * 32 + li];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      if (fw + 32 * a < d) {  // wave-uniform
        const int ft = fw + 32 * a + li;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float yv = a == 0 ? y0v[i] : (ft < d ? Y[(size_t)min(y0 + 16 * h + i, NY - 1) * d + ft] : 0.f);
          acc[a] = tile_mfma(ga[i], yv, acc[a]);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    const int ft = fw + 32 * a + li;
    if (ft < d) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int xi = x0 + tile_row(r, h);
        if (xi < NX) {
          float* p = out + (size_t)xi * d + ft;
          *p = ACCUM ? *p + acc[a][r] : acc[a][r];
        }
      }
    }
  }
}

// ---- host side of the walk
// grid_x, feat_chunk and grid_y of a plan struct for `own` rows of d features: 512 features per workgroup where that
// gives every compute unit one; else 128: four times the workgroups
template <class Plan>
void tile_grad_plan(Plan& p, int own, int d) {
  p.grid_x = (unsigned)((own + 31) / 32);
  p.feat_chunk = (long long)p.grid_x * ((d + TILE_FEAT - 1) / TILE_FEAT) >= 256 ? TILE_FEAT : TILE_FEAT / 4;
  p.grid_y = (unsigned)((d + p.feat_chunk - 1) / p.feat_chunk);
}
// LDS of a kernel built on the walk; `extra_words`: what the kernel declares beside it
constexpr unsigned tile_grad_lds_bytes(int extra_words = 0) {
  return (unsigned)((2 * 32 * TILE_KST + 4 * 32 * TILE_PS + 32 * 32 + extra_words) * sizeof(float));
}
// Launches KERNEL<OWN, ACCUM, NACC> (a kernel built on the walk) on a plan filled by tile_grad_plan: NACC by the plan's
// feat_chunk; TILE_GRAD_LAUNCH takes ACCUM as a run-time flag, TILE_GRAD_LAUNCH_NACC as a constant (and instantiates
// only that one).
#define TILE_GRAD_LAUNCH_NACC(KERNEL, OWN, ACCUM, plan, stream, ...)                                                        \
  do {                                                                                                                     \
    if ((plan).feat_chunk == TILE_FEAT)                                                                                    \
      hipLaunchKernelGGL((KERNEL<OWN, ACCUM, 4>), dim3((plan).grid_x, (plan).grid_y), dim3((plan).block), 0, stream,        \
                         __VA_ARGS__);                                                                                     \
    else                                                                                                                   \
      hipLaunchKernelGGL((KERNEL<OWN, ACCUM, 1>), dim3((plan).grid_x, (plan).grid_y), dim3((plan).block), 0, stream,        \
                         __VA_ARGS__);                                                                                     \
  } while (0)
#define TILE_GRAD_LAUNCH(KERNEL, OWN, accum, plan, stream, ...)                            \
  do {                                                                                     \
    if (accum) TILE_GRAD_LAUNCH_NACC(KERNEL, OWN, true, plan, stream, __VA_ARGS__);        \
    else TILE_GRAD_LAUNCH_NACC(KERNEL, OWN, false, plan, stream, __VA_ARGS__);             \
  } while (0)

}  // namespace
}  // namespace clipfs
