// Merged weights:  out = W + scale * B A  for a whole TABLE of adapted projections in one launch (clipfs_lora_merge).
// The reference folds an adapter into its weight when a layer goes to eval mode (LoRALayer.merge_BA / add_lora_data,
// lora_train_vlp.py:218-234) and writes the master weight; here W is read only and the sum lands in a copy, with the
// copy's 16-bit image (clipfs_convert_f16 / clipfs_split_bf16, bit for bit: convert16.h) written in the same pass.
//
// The kernel is HBM-bound (W in, out and 0.5 - 1 x planes out, r FMAs per element in between): no matrix cores, 16-byte
// loads and stores.  A workgroup owns one tile of TILE_ROWS x TILE_COLS elements of one segment of one job and finds
// the job from the tile prefix (tile0) carried in the table: every thread looks at one record, an LDS max picks the
// last job that starts at or before the workgroup's index.  The tile's r x TILE_COLS slice of A and its TILE_ROWS x r
// slice of B are staged in LDS once, so A comes from L2 once per tile, not once per row.  A thread owns 4 rows x 8
// columns: per rank step two 16-byte LDS reads of A feed 32 FMAs, and the rows' B values are read four ranks at a time.
// The rank sum is sequential (ascending j, one fused multiply-add per step), never split and never atomic, so a result
// depends on nothing but its inputs.
#include "common.h"
#include "convert16.h"

#include <limits.h>

namespace clipfs {

constexpr int MERGE_TR = CLIPFS_LORA_MERGE_TILE_ROWS;  // 32: 8 thread rows x 4
constexpr int MERGE_TC = CLIPFS_LORA_MERGE_TILE_COLS;  // 256: 32 thread columns x 8
constexpr int MERGE_RMAX = 64;
static_assert(MERGE_TR == 32 && MERGE_TC == 256, "the thread mapping below is written for 32 x 256 tiles");

typedef clipfs_lora_merge_job MergeJob;

__host__ __device__ inline int merge_job_tiles(int n, int k, int nseg) {
  return nseg * ((n / nseg + MERGE_TR - 1) / MERGE_TR) * ((k + MERGE_TC - 1) / MERGE_TC);
}

__device__ __forceinline__ f32x4 fma4(float b, const f32x4& a, const f32x4& c) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf(b, a[e], c[e]);
  return o;
}

// FMT: 0 no planes, 1 bf16 hi / lo, 2 f16
template <int FMT>
__global__ __launch_bounds__(256, 4) void lora_merge_kernel(const MergeJob* __restrict__ jobs, int njobs, int r, float scale) {
  extern __shared__ __attribute__((aligned(16))) float merge_smem[];
  __shared__ int s_job;
  const int tid = threadIdx.x, bid = blockIdx.x;
  if (tid == 0) s_job = 0;
  __syncthreads();
  for (int i = tid; i < njobs; i += 256)
    if (jobs[i].tile0 <= bid) atomicMax(&s_job, i);
  __syncthreads();
  const MergeJob jb = jobs[s_job];
  const int n = jb.n, k = jb.k, nseg = jb.nseg;
  // the host validated these bytes; a table that differs from it writes nothing rather than out of bounds
  if (n <= 0 || k <= 0 || (nseg != 1 && nseg != 3) || n % nseg != 0 || (k & 7)) return;
  const int t = bid - jb.tile0;
  if (t < 0 || t >= merge_job_tiles(n, k, nseg)) return;
  const int segrows = n / nseg;
  const int rts = (segrows + MERGE_TR - 1) / MERGE_TR, cts = (k + MERGE_TC - 1) / MERGE_TC;
  const int rt = t / cts, g = rt / rts;
  const int col0 = (t - rt * cts) * MERGE_TC;
  const int row_lo = g * segrows + (rt - g * rts) * MERGE_TR;
  const int row_hi = min(g * segrows + segrows, row_lo + MERGE_TR);
  const bool adapt = (jb.seg_mask >> g) & 1u;  // the same for the whole workgroup
  const int rp = (r + 3) & ~3;                 // row stride of the B slice: 16-byte aligned rows
  float* sA = merge_smem;                      // [r][256]: float4 c4 of a row at slot (c4 & 1) * 32 + (c4 >> 1)
  float* sB = merge_smem + r * MERGE_TC;       // [32][rp]

  // W first: its loads are in flight while the adapter slices are staged
  const int tx = tid & 31, ty = tid >> 5;
  const int col = col0 + tx * 8;  // k % 8 == 0: a thread's 8 columns are all inside or all outside
  const bool active = col < k;
  f32x4 w0[4], w1[4], acc0[4], acc1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row_lo + ty + 8 * i;
    w0[i] = w1[i] = acc0[i] = acc1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active && row < row_hi) {
      const float* wp = jb.w + (size_t)row * k + col;
      w0[i] = *reinterpret_cast<const f32x4*>(wp);
      w1[i] = *reinterpret_cast<const f32x4*>(wp + 4);
    }
  }

  if (adapt) {
    const float* A = jb.a + (size_t)g * r * k;
    for (int idx = tid; idx < r * (MERGE_TC / 4); idx += 256) {
      const int j = idx >> 6, c4 = idx & 63, ca = col0 + c4 * 4;
      if (ca < k)
        *reinterpret_cast<f32x4*>(sA + j * MERGE_TC + (((c4 & 1) << 5) + (c4 >> 1)) * 4) =
            *reinterpret_cast<const f32x4*>(A + (size_t)j * k + ca);
    }
    const float* Bp = jb.b + (size_t)row_lo * r;  // the tile's rows of B are contiguous
    const int nb = (row_hi - row_lo) * r;
    if ((r & 3) == 0) {
      for (int idx = tid; idx < nb / 4; idx += 256)
        reinterpret_cast<f32x4*>(sB)[idx] = reinterpret_cast<const f32x4*>(Bp)[idx];
    } else {
      for (int idx = tid; idx < nb; idx += 256) {
        const int rl = idx / r;
        sB[rl * rp + (idx - rl * r)] = Bp[idx];
      }
    }
    __syncthreads();
  }

  if (!active) return;
  if (adapt) {
    const float* a_thr = sA + tx * 4;
    int j = 0;
    for (; j + 4 <= r; j += 4) {
      f32x4 bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) bv[i] = *reinterpret_cast<const f32x4*>(sB + (ty + 8 * i) * rp + j);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(a_thr + (j + jj) * MERGE_TC);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(a_thr + (j + jj) * MERGE_TC + 128);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc0[i] = fma4(bv[i][jj], a0, acc0[i]);
          acc1[i] = fma4(bv[i][jj], a1, acc1[i]);
        }
      }
    }
    for (; j < r; ++j) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a_thr + j * MERGE_TC);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(a_thr + j * MERGE_TC + 128);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float b = sB[(ty + 8 * i) * rp + j];
        acc0[i] = fma4(b, a0, acc0[i]);
        acc1[i] = fma4(b, a1, acc1[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row_lo + ty + 8 * i;
    if (row >= row_hi) continue;
    f32x4 o0 = w0[i], o1 = w1[i];  // a segment without an adapter: the bits of W
    if (adapt) {
      o0 = fma4(scale, acc0[i], w0[i]);
      o1 = fma4(scale, acc1[i], w1[i]);
    }
    const size_t off = (size_t)row * k + col;
    *reinterpret_cast<f32x4*>(jb.out + off) = o0;
    *reinterpret_cast<f32x4*>(jb.out + off + 4) = o1;
    if (FMT == 2 && jb.planes) {
      *reinterpret_cast<f16x8*>(reinterpret_cast<_Float16*>(jb.planes) + off) = to_f16x8(o0, o1);
    } else if (FMT == 1 && jb.planes) {
      __bf16* hi = reinterpret_cast<__bf16*>(jb.planes);
      bf16x8 h, l;
      split8(o0, o1, h, l);
      *reinterpret_cast<bf16x8*>(hi + off) = h;
      *reinterpret_cast<bf16x8*>(hi + (size_t)n * k + off) = l;
    }
  }
}

template <int FMT>
static int launch_merge(const MergeJob* jobs_dev, int njobs, int tiles, int r, float scale, hipStream_t stream) {
  const size_t lds = ((size_t)r * MERGE_TC + (size_t)MERGE_TR * ((r + 3) & ~3)) * sizeof(float);
  static bool attr = false;
  if (!attr && lds > 48 * 1024) {  // r = 64 needs 72 KB
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lora_merge_kernel<FMT>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (MERGE_RMAX * MERGE_TC + MERGE_TR * MERGE_RMAX) * (int)sizeof(float));
    attr = true;
  }
  hipLaunchKernelGGL(lora_merge_kernel<FMT>, dim3(tiles), dim3(256), lds, stream, jobs_dev, njobs, r, scale);
  return launch_status();
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_lora_merge(const clipfs_lora_merge_job* h_jobs, const clipfs_lora_merge_job* jobs_dev, int njobs,
                                 size_t struct_size, int r, float scale, int plane_format, void* stream) {
  CLIPFS_REQUIRE(struct_size == sizeof(clipfs_lora_merge_job),
                 "lora_merge: struct_size %zu is not sizeof(clipfs_lora_merge_job) = %zu of this library", struct_size,
                 sizeof(clipfs_lora_merge_job));
  CLIPFS_REQUIRE(h_jobs && jobs_dev, "lora_merge: null job table (host %p, device %p)", (const void*)h_jobs,
                 (const void*)jobs_dev);
  CLIPFS_REQUIRE(njobs > 0 && njobs <= 65536, "lora_merge: njobs %d (must be in [1, 65536])", njobs);
  CLIPFS_REQUIRE(r >= 1 && r <= MERGE_RMAX, "lora_merge: r %d (must be in [1, %d])", r, MERGE_RMAX);
  CLIPFS_REQUIRE(plane_format >= 0 && plane_format <= 2, "lora_merge: plane_format %d (0 none, 1 bf16 hi/lo, 2 f16)",
                 plane_format);
  CLIPFS_REQUIRE(aligned16(jobs_dev), "lora_merge: the device job table is not 16-byte aligned");
  long long tiles = 0;
  for (int i = 0; i < njobs; ++i) {
    const clipfs_lora_merge_job& j = h_jobs[i];
    CLIPFS_REQUIRE(j.w, "lora_merge: job %d: w is NULL", i);
    CLIPFS_REQUIRE(j.a, "lora_merge: job %d: a is NULL", i);
    CLIPFS_REQUIRE(j.b, "lora_merge: job %d: b is NULL", i);
    CLIPFS_REQUIRE(j.out, "lora_merge: job %d: out is NULL", i);
    CLIPFS_REQUIRE(aligned16(j.w), "lora_merge: job %d: w is not 16-byte aligned", i);
    CLIPFS_REQUIRE(aligned16(j.a), "lora_merge: job %d: a is not 16-byte aligned", i);
    CLIPFS_REQUIRE(aligned16(j.b), "lora_merge: job %d: b is not 16-byte aligned", i);
    CLIPFS_REQUIRE(aligned16(j.out), "lora_merge: job %d: out is not 16-byte aligned", i);
    CLIPFS_REQUIRE(aligned16(j.planes), "lora_merge: job %d: planes is not 16-byte aligned", i);
    CLIPFS_REQUIRE(!j.planes || plane_format != 0, "lora_merge: job %d: planes given with plane_format 0", i);
    CLIPFS_REQUIRE(j.out != j.w, "lora_merge: job %d: out aliases w (the master weight is never written)", i);
    CLIPFS_REQUIRE(j.n > 0 && j.k > 0 && (long long)j.n * j.k <= INT_MAX, "lora_merge: job %d: n %d, k %d", i, j.n, j.k);
    CLIPFS_REQUIRE(j.k % 8 == 0, "lora_merge: job %d: k %d is not a multiple of 8", i, j.k);
    CLIPFS_REQUIRE(j.nseg == 1 || j.nseg == 3, "lora_merge: job %d: nseg %d (must be 1 or 3)", i, j.nseg);
    CLIPFS_REQUIRE(j.n % j.nseg == 0, "lora_merge: job %d: n %d is not a multiple of nseg %d", i, j.n, j.nseg);
    CLIPFS_REQUIRE(j.seg_mask != 0 && (j.seg_mask >> j.nseg) == 0, "lora_merge: job %d: seg_mask 0x%x (non-zero, inside %d bits)",
                   i, j.seg_mask, j.nseg);
    CLIPFS_REQUIRE(j.tile0 == tiles, "lora_merge: job %d: tile0 %d, the jobs before it have %lld tiles", i, j.tile0, tiles);
    CLIPFS_REQUIRE(j.reserved == 0, "lora_merge: job %d: reserved %d (must be 0)", i, j.reserved);
    tiles += merge_job_tiles(j.n, j.k, j.nseg);
    CLIPFS_REQUIRE(tiles <= INT_MAX, "lora_merge: job %d: the table has more than %d tiles", i, INT_MAX);
  }
  hipStream_t st = (hipStream_t)stream;
  if (plane_format == 2) return launch_merge<2>(jobs_dev, njobs, (int)tiles, r, scale, st);
  if (plane_format == 1) return launch_merge<1>(jobs_dev, njobs, (int)tiles, r, scale, st);
  return launch_merge<0>(jobs_dev, njobs, (int)tiles, r, scale, st);
}
