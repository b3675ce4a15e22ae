// fp32 "NT" GEMM on the CDNA4 matrix cores:  C[M,N] = epi( alpha * A[M,K] * B[N,K]^T ).
//
// v_mfma_f32_32x32x2_f32 (exact f32, k-ordered fma chain) -- the only MFMA that meets the
// 1e-3-on-100x-cosine-logits budget of the north star (SURVEY.md section 7 "hard parts").
//
// Block tile BM x BN x 32, 256 threads = 4 waves (2 x 2), wave tile (BM/2) x (BN/2) made of
// 32x32 MFMA tiles.  Both operands are K-contiguous in memory, so a staging thread moves 16-byte
// K-chunks: global -> registers (issued one K-step ahead) -> LDS (double buffered, one barrier
// per K-step).  LDS image per operand: [rows][32 floats] with the 16-byte chunk index XOR-swizzled
// by (row >> 1) & 7, which makes both the ds_write_b128 of the staging pass and the ds_read_b128 of
// the fragment reads bank-conflict free (read groups are 16 lanes of distinct rows; MI355X_MICROARCH
// "LDS").  A lane's 4 consecutive k values feed 4 successive MFMAs: MFMA e of k-group q multiplies
// k = 8q+e (lanes 0-31) and k = 8q+4+e (lanes 32-63) -- any pairing is legal as long as A and B agree.
//
// Ragged M and N are handled by clamping the staged row index and predicating the stores; a K tail
// (K % 32 != 0) is zero filled.  Epilogue order is documented in include/clipfs.h.
#include "common.h"
#include "gemm_common.h"

#include <stdlib.h>

#include <vector>

// Timing-only ablations of the register-staging K loop (skip the prefetch / the LDS stores / the barrier: WRONG results) exist only in a diagnostic build: `HIPCC_EXTRA=-DCLIPFS_ABLATION_BUILD python build.py --force`, then
// CLIPFS_GEMM_ABLATE=<bits> (scripts/ablate_gemm.py).  The shipped library compiles them out.
#ifdef CLIPFS_ABLATION_BUILD
#define CLIPFS_ABLATE(mask, bit) ((mask) & (bit))
#else
#define CLIPFS_ABLATE(mask, bit) 0
#endif

#ifdef CLIPFS_STAMPS
// Diagnostic build only (HIPCC_EXTRA=-DCLIPFS_STAMPS, build.py --tag stamps): s_memtime at four points of every
// workgroup of gemm_nt_kernel + the hardware ids of the CU it ran on, written to a buffer nothing else reads
// (scripts/gemm_stamps.py).
__device__ unsigned long long clipfs_gemm_stamps[16384 * 6];
#define CLIPFS_STAMP(i)                                                                                     \
  do {                                                                                                      \
    if (threadIdx.x == 0 && blockIdx.x < 16384) {                                                           \
      clipfs_gemm_stamps[blockIdx.x * 6 + (i)] = __builtin_amdgcn_s_memtime();                              \
      if ((i) == 1) clipfs_gemm_stamps[blockIdx.x * 6 + 4] = __builtin_amdgcn_s_memrealtime();              \
      if ((i) == 2) clipfs_gemm_stamps[blockIdx.x * 6 + 5] = __builtin_amdgcn_s_memrealtime();              \
      if (0) {                                                                                       \
        unsigned hw, xcc;                                                                                   \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                  \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                                \
        clipfs_gemm_stamps[blockIdx.x * 6 + 4] = hw;                                                        \
        clipfs_gemm_stamps[blockIdx.x * 6 + 5] = xcc;                                                       \
      }                                                                                                     \
    }                                                                                                       \
  } while (0)
extern "C" int clipfs_debug_read_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(clipfs_gemm_stamps), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
#else
#define CLIPFS_STAMP(i) do {} while (0)
#endif

namespace clipfs {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // first-class vector: stays in VGPRs (HIP's float4 struct arrays went to scratch)
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));

// 16-byte global -> LDS copy without a VGPR round trip (global_load_lds_dwordx4): the LDS destination is
// wave-uniform base + lane * 16, the global source is per lane -- so the XOR swizzle goes on the SOURCE.
__device__ __forceinline__ void glds16(const float* gsrc, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// AMODE 0: dense A, K % 32 == 0 (the hot configuration: the K loop is pointer bumps + 16-byte loads only)
// AMODE 1: patch im2col with patch == 32 (one K-step == one (channel, ky) image row segment)
// AMODE 2: generic (dense with a K tail, or any patch size): per-element address arithmetic
//
// gemm_nt_tile is one workgroup's whole job: the BM x BN tile at (m0, n0), K slice `split` of tile number `tile` (both
// only matter when p.splits > 1).  The kernels below differ in how a workgroup finds its tile.
template <int BM, int BN, int AMODE>
__device__ __forceinline__ void gemm_nt_tile(const GemmParams& p, const int tile, const int split, const int m0, const int n0) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int WM = BM >= 64 ? 2 : 1;   // wave grid WM x WN (4 waves); BM = 32 puts the 4 waves side by side
  constexpr int WN = 4 / WM;
  constexpr int TM = BM / (32 * WM);     // 32x32 tiles per wave along M
  constexpr int TN = BN / (32 * WN);     // ... along N
  constexpr int A_CHUNKS = BM * 8 / 256; // 16-byte chunks staged per thread
  constexpr int B_CHUNKS = BN * 8 / 256;
  constexpr int STAGE_FLOATS = (BM + BN) * BK;

  const clipfs_gemm_args& g = p.a;
  CLIPFS_STAMP(0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int M = g.M, N = g.N, K = g.K;

  // ---- staging addresses -------------------------------------------------------------------
  const float* a_src[A_CHUNKS];
  int a_lds[A_CHUNKS];
  const int kc = tid & 7;  // chunk (4 floats) inside the 32-wide K-step, same for every chunk id
#pragma unroll
  for (int i = 0; i < A_CHUNKS; ++i) {
    const int row = (tid >> 3) + 32 * i;
    const int m = min(m0 + row, M - 1);
    if (AMODE == 0 || AMODE == 3 || (AMODE == 2 && g.a_mode == 0)) {
      a_src[i] = g.A + (size_t)m * g.lda + (AMODE == 0 ? kc * 4 : 0);
    } else {
      const int b = m / p.patches, pp = m - b * p.patches;
      const int py = pp / p.grid_g, px = pp - py * p.grid_g;
      a_src[i] = g.A + ((size_t)b * 3 * g.img_res + (size_t)py * g.patch) * g.img_res + (size_t)px * g.patch +
                 (AMODE == 1 ? kc * 4 : 0);
    }
    a_lds[i] = row * BK + ((kc ^ ((row >> 1) & 7)) << 2);
  }
  const float* b_src[B_CHUNKS];
  int b_lds[B_CHUNKS];
#pragma unroll
  for (int i = 0; i < B_CHUNKS; ++i) {
    const int row = (tid >> 3) + 32 * i;
    const int n = min(n0 + row, N - 1);
    b_src[i] = g.B + (size_t)n * g.ldb + (AMODE != 2 ? kc * 4 : 0);
    b_lds[i] = BM * BK + row * BK + ((kc ^ ((row >> 1) & 7)) << 2);
  }

  f32x4 a_reg[A_CHUNKS], b_reg[B_CHUNKS];
  auto load_global = [&](int kt) __attribute__((always_inline)) {
    if (AMODE == 0 || AMODE == 3) {
      const int k0 = kt * BK;
#pragma unroll
      for (int i = 0; i < A_CHUNKS; ++i) a_reg[i] = *reinterpret_cast<const f32x4*>(a_src[i] + k0);
#pragma unroll
      for (int i = 0; i < B_CHUNKS; ++i) b_reg[i] = *reinterpret_cast<const f32x4*>(b_src[i] + k0);
    } else if (AMODE == 1) {
      // patch == 32 == BK: K-step kt is image row (c = kt / 32, ky = kt % 32) of every patch
      const int k0 = kt * BK;
      const size_t off = ((size_t)(kt >> 5) * g.img_res + (kt & 31)) * g.img_res;
#pragma unroll
      for (int i = 0; i < A_CHUNKS; ++i) a_reg[i] = *reinterpret_cast<const f32x4*>(a_src[i] + off);
#pragma unroll
      for (int i = 0; i < B_CHUNKS; ++i) b_reg[i] = *reinterpret_cast<const f32x4*>(b_src[i] + k0);
    } else {
      const int k = kt * BK + kc * 4;
      const bool k_ok = k < K;  // K % 4 == 0 is checked on the host
      if (g.a_mode == 0) {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i)
          a_reg[i] = k_ok ? *reinterpret_cast<const f32x4*>(a_src[i] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        const int pp2 = g.patch * g.patch;
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
          float t[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kk = k + e;
            const int c2 = kk / pp2, r2 = kk - c2 * pp2;
            const int ky2 = r2 / g.patch, kx2 = r2 - ky2 * g.patch;
            t[e] = kk < K ? a_src[i][((size_t)c2 * g.img_res + ky2) * g.img_res + kx2] : 0.f;
          }
          a_reg[i] = f32x4{t[0], t[1], t[2], t[3]};
        }
      }
#pragma unroll
      for (int i = 0; i < B_CHUNKS; ++i)
        b_reg[i] = k_ok ? *reinterpret_cast<const f32x4*>(b_src[i] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto store_lds = [&](int stage) __attribute__((always_inline)) {
    float* s = smem + stage * STAGE_FLOATS;
#pragma unroll
    for (int i = 0; i < A_CHUNKS; ++i) *reinterpret_cast<f32x4*>(s + a_lds[i]) = a_reg[i];
#pragma unroll
    for (int i = 0; i < B_CHUNKS; ++i) *reinterpret_cast<f32x4*>(s + b_lds[i]) = b_reg[i];
  };

  // ---- AMODE 3: dense operands copied global -> LDS directly (no VGPR staging, no ds_write) -------------
  // one global_load_lds_dwordx4 covers 8 tile rows x 128 B = 1 KiB of the LDS image (lane l: row l / 8,
  // slot l % 8); wave w owns row groups w, w + 4, ...; the swizzle is applied to the per-lane SOURCE chunk.
  const float* ga_src[A_CHUNKS];
  const float* gb_src[B_CHUNKS];
  int ga_lds[A_CHUNKS], gb_lds[B_CHUNKS];
  if (AMODE == 3) {
    const int uw = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
    for (int i = 0; i < A_CHUNKS; ++i) {
      const int r0 = 8 * (uw + 4 * i), r = r0 + (lane >> 3);
      const int c = (lane & 7) ^ ((r >> 1) & 7);
      ga_src[i] = g.A + (size_t)min(m0 + r, M - 1) * g.lda + 4 * c;
      ga_lds[i] = r0 * BK;
    }
#pragma unroll
    for (int i = 0; i < B_CHUNKS; ++i) {
      const int r0 = 8 * (uw + 4 * i), r = r0 + (lane >> 3);
      const int c = (lane & 7) ^ ((r >> 1) & 7);
      gb_src[i] = g.B + (size_t)min(n0 + r, N - 1) * g.ldb + 4 * c;
      gb_lds[i] = BM * BK + r0 * BK;
    }
  }
  auto glds_stage = [&](int kt, int stage) __attribute__((always_inline)) {
    float* s = smem + stage * STAGE_FLOATS;
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < A_CHUNKS; ++i) glds16(ga_src[i] + k0, s + ga_lds[i]);
#pragma unroll
    for (int i = 0; i < B_CHUNKS; ++i) glds16(gb_src[i] + k0, s + gb_lds[i]);
  };

  // ---- fragment read addresses -----------------------------------------------------------------
  const int fr = lane & 31, fh = lane >> 5;
  const int swz = (fr >> 1) & 7;  // (row >> 1) & 7 : tile bases are multiples of 32
  int a_frag[TM], b_frag[TN];
#pragma unroll
  for (int t = 0; t < TM; ++t) a_frag[t] = (wm * (BM / WM) + t * 32 + fr) * BK;
#pragma unroll
  for (int t = 0; t < TN; ++t) b_frag[t] = BM * BK + (wn * (BN / WN) + t * 32 + fr) * BK;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk_all = (K + BK - 1) / BK;
  const int kt0 = (int)((long)split * nk_all / p.splits);
  const int nk = (int)((long)(split + 1) * nk_all / p.splits) - kt0;  // K-steps of this unit (>= 1: host guarantees)
  auto compute = [&](const float* s) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ch = (((2 * q + fh) ^ swz) << 2);
      f32x4 av[TM], bv[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) av[t] = *reinterpret_cast<const f32x4*>(s + a_frag[t] + ch);
#pragma unroll
      for (int t = 0; t < TN; ++t) bv[t] = *reinterpret_cast<const f32x4*>(s + b_frag[t] + ch);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float ae = av[i][e];
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const float be = bv[j][e];
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae, be, acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  };
  if (AMODE == 3) {
    glds_stage(kt0, 0);
    __syncthreads();  // emits vmcnt(0) for the LDS-DMA in flight, then the barrier
    CLIPFS_STAMP(1);
    for (int kt = 0; kt + 1 < nk; ++kt) {
      glds_stage(kt0 + kt + 1, (kt + 1) & 1);  // the other stage was last read before the previous barrier
      compute(smem + (kt & 1) * STAGE_FLOATS);
      __syncthreads();
    }
    compute(smem + ((nk - 1) & 1) * STAGE_FLOATS);
  } else {
  // prologue, steady state (prefetch unconditionally: the staged registers must stay in VGPRs), tail
  load_global(kt0);
  store_lds(0);
  __syncthreads();
  for (int kt = 0; kt + 1 < nk; ++kt) {
    if (!CLIPFS_ABLATE(p.ablate, 1)) load_global(kt0 + kt + 1);  // global -> registers, one K-step ahead
    __builtin_amdgcn_sched_barrier(0);         // keep the loads ABOVE the MFMAs (hipcc sinks them to the ds_write otherwise)
    compute(smem + (kt & 1) * STAGE_FLOATS);   // 32 MFMAs per wave hide the load latency
    if (!CLIPFS_ABLATE(p.ablate, 2)) store_lds((kt + 1) & 1);  // registers -> the other LDS stage
    if (!CLIPFS_ABLATE(p.ablate, 4)) __syncthreads();
  }
  compute(smem + ((nk - 1) & 1) * STAGE_FLOATS);
  }

  CLIPFS_STAMP(2);
  // ---- LoRA up-projection on the matrix cores + epilogue (gemm_common.h) ------------------------------------
  if (p.splits > 1) {
    // Split-K without a combine launch: every K slice publishes its raw accumulators as a slab (register order: one
    // 16-byte store per lane, fully coalesced) WRITE-THROUGH (sc1), takes a ticket on the tile's arrival counter, and
    // the slice that arrives LAST adds the slabs in slice order -- bitwise reproducible whatever the arrival order --
    // and runs the same LoRA + epilogue code as an unsplit tile.  Nobody waits, so no residency assumption; every slab
    // load is an sc1 load (bypasses this CU's L1, which no other CU's store refreshes): no release / acquire fence
    // (MI355X_MICROARCH.md "Valid forms").  The counter is left zero.
    constexpr int SLAB = BM * BN;
    const int S = p.splits;
    {
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(p.part + ((size_t)tile * S + split) * SLAB, 0, SLAB * 4, 0x00020000);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const f32x4 val = f32x4{acc[i][j][4 * v], acc[i][j][4 * v + 1], acc[i][j][4 * v + 2], acc[i][j][4 * v + 3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, val), rs,
                                                   (((i * TN + j) * 4 + v) * 256 + tid) * 16, 0, /*sc1*/ 16);
          }
    }
    int* flag = reinterpret_cast<int*>(smem + 2 * STAGE_FLOATS);  // one word behind the two stages (the host adds it)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its write-through stores ...
    __syncthreads();                                    // ... before ONE lane signals (also: everybody is done with the stages)
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(p.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == S - 1;
      if (last) __hip_atomic_store(p.cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *flag = last;
    }
    __syncthreads();
    if (!*flag) return;
    if (S > 2) {  // (s0 + s1) + s2 + ...: every slab from memory, the own one included (it was stored write-through)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }
    for (int c = 0; c < S; ++c) {
      if (S == 2 && c == split) continue;  // two slices: a + b == b + a, the own slab stays in registers
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(p.part + ((size_t)tile * S + c) * SLAB, 0, SLAB * 4, 0x00020000);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          f32x4 u[4];
#pragma unroll
          for (int v = 0; v < 4; ++v)
            u[v] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 rs, (((i * TN + j) * 4 + v) * 256 + tid) * 16, 0, /*sc1*/ 16));
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][4 * v + e] += u[v][e];
        }
    }
  }
  finish_tiles<TM, TN>(g, p.patches, acc, m0 + wm * (BM / WM), n0 + wn * (BN / WN), m0 + BM <= M && n0 + BN <= N, lane);
  CLIPFS_STAMP(3);
}

// Tile order.  Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the XCD, speed only),
// each XCD has a private 4 MB L2: give every XCD a CONTIGUOUS run of the tile list (unit `bid` of `nwg`), and order
// the list in super-tiles of GM m-blocks x all n-blocks (m fastest) so the ~96 tiles an XCD runs at once share
// 8 A panels and 12 B panels instead of ~40 + 18 (FETCH_SIZE: DESIGN.md section 8; GM = 8 fetches 10-25 % less than
// 16 on four of the five path shapes, 4 and 32 more; the time does not move: the kernel is MFMA-bound).
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
  const int xcd = bid & 7, li = bid >> 3, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + li;
}

// block coordinates of tile number `tile` among mb_total x nbn blocks
__device__ __forceinline__ void tile_blocks(int tile, int GM, int nbn, int mb_total, int& mb, int& nb) {
  const int grp = tile / (GM * nbn);
  const int rem = tile - grp * (GM * nbn);
  const int gm = min(GM, mb_total - grp * GM);  // the last group may be shorter
  mb = grp * GM + rem % gm;
  nb = rem / gm;
}

template <int BM, int BN, int AMODE>
__global__ __launch_bounds__(256) void gemm_nt_kernel(const GemmParams p) {
  int tile = xcd_contiguous(blockIdx.x, gridDim.x);
  const int split = tile % p.splits;  // consecutive units = the K slices of one tile (same XCD: shared panels)
  tile /= p.splits;
  int mb, nb;
  tile_blocks(tile, p.gm, p.n_blocks_n, (p.a.M + BM - 1) / BM, mb, nb);
  gemm_nt_tile<BM, BN, AMODE>(p, tile, split, mb * BM, nb * BN);
}

// Two tile heights in one launch (dense operands, unsplit): rows [0, mix_rows64) as mix_tiles64 tiles of 64 x 128 --
// whole rounds of the resident workgroup slots, dispatched first -- and the rows behind them as 32 x 128 tiles that
// fill the last round.  The branch is per workgroup; an element's k order does not depend on the tile that holds it,
// so the result is bitwise that of either uniform tiling.
__global__ __launch_bounds__(256) void gemm_nt_mixed_kernel(const GemmParams p) {
  const int bid = blockIdx.x, t64 = p.mix_tiles64;
  int mb, nb;
  if (bid < t64) {
    tile_blocks(xcd_contiguous(bid, t64), p.gm, p.n_blocks_n, p.mix_rows64 / 64, mb, nb);
    gemm_nt_tile<64, 128, 3>(p, 0, 0, mb * 64, nb * 128);
  } else {
    tile_blocks(xcd_contiguous(bid - t64, gridDim.x - t64), p.gm, p.n_blocks_n, (p.a.M - p.mix_rows64 + 31) / 32, mb, nb);
    gemm_nt_tile<32, 128, 3>(p, 0, 0, p.mix_rows64 + mb * 32, nb * 128);
  }
}

// ---- optional per-launch timing (bench.py roofline leg): HIP events on the launch stream around every
// GEMM while enabled.  Off by default; never on in the timed region.
struct TimedLaunch {
  hipEvent_t start, stop;
  double flops;
  double bytes;  // algorithmic HBM bytes: each operand, result and epilogue tensor touched once
};
static thread_local double g_last_bytes = 0.0;
static thread_local bool g_timing = false;
static thread_local std::vector<TimedLaunch>* g_timed = nullptr;

}  // namespace clipfs

using namespace clipfs;

// ---- the schedule: the ONE place that decides tiles, split-K, the band, grids and LDS sizes ---------------------------
// clipfs_gemm_plan and clipfs_gemm_nt execute it for a call's route; the shape-only queries of clipfs.h are its answers
// for a dense fp32 product with scratch.  Stated for the MI355X: 256 CUs, two resident workgroups on each.
//
// Tile height: 64 x 128, or 32 x 128 when that balances the 256 CUs better.  All tiles of a launch that fits the
// resident slots start together and share their CU's MFMA pipe, so a launch lasts ceil(tiles / 256) tile-times of
// the busiest CU: cost = ceil(tiles / 256) * rows-per-tile, with 8 % on top for the 32-row tile (one LDS read per 2
// MFMAs instead of 3 per 8, 1.67 x the LDS-DMA bytes per FLOP).  The 8 % was measured on the per-rank shapes of the
// strong-scaling run (scripts/bench_small_m.py): e.g. 600 tiles of 64 rows (3 vs 2.34 per CU) lose 7-9 % against 1200
// tiles of 32 rows, 450 tiles of 64 rows win by 9 %.
//
// Split-K: only when even the chosen tiling leaves the 512 slots short of work (strong-scaling per-rank batches, the
// one-row-per-sequence products of the last block) and K is long enough to cut.  The slices of a tile are combined by
// the last one to arrive inside the same launch (no second kernel), so the factor aims at ~one unit per slot, with at
// least 4 K-steps per unit.  It needs the slab scratch AND the (caller-zeroed) arrival counters.
//
// The large-M band: where the cost model picks 32 rows for a dense unsplit product of BAND_MIN_M rows or more (the
// packed text tower's N = 512 products on ~10 k live rows: 4.8 32-row tiles per slot), most of the launch is whole
// rounds of tiles and only the last round needs the finer balance.  The rows of the whole rounds of the 512 slots are
// dealt as 64 x 128 tiles (3 LDS reads per 8 MFMAs against 4, and 0.6 x the LDS-DMA bytes per FLOP of the 32-row tile)
// and only the rows behind them as 32 x 128 tiles, in one launch (gemm_nt_mixed_kernel).  [9748, 512]: 512 + 196
// workgroups; the busiest CU does 2 x 64 + 1.08 x 32 = 163 row-units against 173 (all 32-row) and 192 (all 64-row).
// Measured on MI355X (profiles/text_band): 3-7 % on each N = 512 product alone, 0.5 ms of the 52.6 ms step.  The
// per-rank shapes, every split product and every shape of the schedule table (tests/gemm_matrix_cases.py) lie below it.
//
// Dynamic LDS of the fp32 kernels: 8 KiB (CLIPFS_GEMM_LDS_PAD) more than the two stages need: two workgroups per CU
// instead of three.  The K loop is as fast with two (the MFMA pipe is the shared resource either way) and the third of
// the CU left free lets the other tower's LayerNorm / attention / LoRA kernels run beside the GEMM: +1.3 % on the step,
// +3.4 % on the 8-GPU per-rank step.
//
// Stream-K (persistent workgroups over tiles x K-steps) and the 128 x 128 / 128 x 64 fp32 tiles were removed at this
// commit: both measured no gain (DESIGN.md sections 3 and 18, profiles/r03).
enum GemmRoute {
  ROUTE_DENSE,    // fp32 operands, a_mode 0, K % 32 == 0 (and what the shape-only queries describe): may split, may mix
  ROUTE_PATCH32,  // 64-row tiles only, never split
  ROUTE_GENERIC,  //   the same
  ROUTE_PLANES,   // gemm_bf16.hip: 64 x 128 or 128 x 128, never split
};

struct GemmSchedule {
  GemmPlan plan;
  int n_blocks_n;   // 128-wide column blocks
  int mix_tiles64;  // MIXED: 64-row tiles (the workgroups in front of the 32-row ones)
};

static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

// planes: 16-bit planes per operand (ROUTE_PLANES).  glds: the dense kernels stage by LDS-DMA (the mixed launch exists
// in that form only).  scratch: the call whose workspace / counters decide whether the split is granted; NULL = enough.
static GemmSchedule gemm_schedule(int M, int N, int K, GemmRoute route, int planes, bool glds, const clipfs_gemm_args* scratch) {
  constexpr long CUS = 256, SLOTS = 2 * CUS;
  constexpr double COST32 = 1.08;                 // a 32-row tile's time per row against a 64-row tile's
  constexpr long SPLIT_BELOW = 384, SPLIT_UNITS = 448;  // split under 3/4 of the slots, towards 7/8 of them
  constexpr int BAND_MIN_M = 4096;
  constexpr long PLANES_BIG_TILES = 1024;         // 128 x 128 plane tiles from this many on
  // tuning aids, read once per process
  static const int force_bm = env_int("CLIPFS_GEMM_BM", 0);          // 32 / 64
  static const int force_splits = env_int("CLIPFS_GEMM_SPLITS", 0);
  static const int gm_cfg = env_int("CLIPFS_GEMM_GM", 8);
  static const int lds_pad = env_int("CLIPFS_GEMM_LDS_PAD", 8);      // KiB
  static const int plane_tile = env_int("CLIPFS_BF16_TILE", 0);      // 1: 128 x 128, 2: 64 x 128

  const long nbn = (N + 127) / 128;
  auto blocks = [](long rows, int bm) { return (rows + bm - 1) / bm; };
  auto cost = [&](long tiles, int bm) { return (double)((tiles + CUS - 1) / CUS) * bm * (bm == 32 ? COST32 : 1.0); };

  GemmSchedule s = {};
  GemmPlan& p = s.plan;
  s.n_blocks_n = (int)nbn;
  p.block = 256;
  p.splits = p.want_splits = 1;
  if (route == ROUTE_PLANES) {
    const bool big = plane_tile == 1 || (plane_tile == 0 && blocks(M, 128) * nbn >= PLANES_BIG_TILES);
    p.kernel = big ? CLIPFS_GEMM_PLANES128 : CLIPFS_GEMM_PLANES64;
    p.planes = planes;
    p.tile_rows = big ? 128 : 64;
    p.gm = 8;  // the plane kernels' constant
    p.grid = (int)(blocks(M, p.tile_rows) * nbn);
    p.lds_bytes = 2 * planes * (p.tile_rows + 128) * 64;  // two stages of 64-byte rows
    return s;
  }
  p.gm = gm_cfg > 0 ? gm_cfg : 8;
  const bool dense = route == ROUTE_DENSE, shape_ok = M > 0 && N > 0 && K > 0;
  const bool cheaper32 = cost(blocks(M, 32) * nbn, 32) < cost(blocks(M, 64) * nbn, 64);
  const int bm = !dense ? 64 : force_bm == 32 || force_bm == 64 ? force_bm : cheaper32 ? 32 : 64;
  const long tiles = blocks(M, bm) * nbn;
  const int nk = (K + BK - 1) / BK;
  if (dense && shape_ok) {
    long want = 1;
    if (force_splits > 0) {
      want = nk >= 2 * force_splits ? force_splits : 1;
    } else if (tiles < SPLIT_BELOW && nk >= 8) {
      want = (SPLIT_UNITS + tiles - 1) / tiles;
      if (want > nk / 4) want = nk / 4;
      if (want > 8) want = 8;
    }
    p.want_splits = (int)want;
  }
  if (p.want_splits > 1) {
    p.workspace_floats = (size_t)p.want_splits * (size_t)tiles * bm * 128;  // one slab of a whole tile per K slice and tile
    p.counter_ints = (size_t)tiles;                                        // one arrival counter per tile
    if (!scratch || (scratch->workspace && scratch->counters && aligned16(scratch->workspace) &&
                     scratch->workspace_floats >= p.workspace_floats && scratch->counters_ints >= p.counter_ints))
      p.splits = p.want_splits;
  }
  long t32 = 0;  // 32-row tiles behind the band's 64-row tiles
  if (dense && glds && shape_ok && p.want_splits == 1 && M >= BAND_MIN_M && (K % BK) == 0 && bm == 32) {
    const long mb64 = (long)(M / 64) * nbn / SLOTS * SLOTS / nbn;  // whole m-blocks inside the whole rounds
    t32 = blocks(M - mb64 * 64, 32) * nbn;
    if (mb64 > 0 && cost(mb64 * nbn, 64) + cost(t32, 32) < cost(tiles, 32)) {
      p.mix_rows64 = (int)(mb64 * 64);
      s.mix_tiles64 = (int)(mb64 * nbn);
    }
  }
  const bool mixed = p.mix_rows64 > 0;
  p.kernel = mixed ? CLIPFS_GEMM_MIXED
             : route == ROUTE_PATCH32 ? CLIPFS_GEMM_PATCH32
             : route == ROUTE_GENERIC ? CLIPFS_GEMM_GENERIC
             : bm == 32 ? CLIPFS_GEMM_NT32
             : glds ? CLIPFS_GEMM_NT64 : CLIPFS_GEMM_NT64_REG;
  p.tile_rows = bm;
  p.grid = (int)(mixed ? s.mix_tiles64 + t32 : tiles * p.splits);
  // the two stages of the tallest tile + the pad + the split-K flag word
  p.lds_bytes = (int)(2 * (size_t)((mixed ? 64 : bm) + 128) * BK * sizeof(float) + (size_t)lds_pad * 1024 + 64);
  return s;
}

static GemmPlan shape_query(int M, int N, int K) { return gemm_schedule(M, N, K, ROUTE_DENSE, 0, true, nullptr).plan; }

extern "C" int clipfs_gemm_tile_rows(int M, int N) { return shape_query(M, N, BK).tile_rows; }
extern "C" int clipfs_gemm_mixed_rows64(int M, int N, int K) { return shape_query(M, N, K).mix_rows64; }
extern "C" int clipfs_gemm_splits(int M, int N, int K) { return shape_query(M, N, K).want_splits; }
extern "C" size_t clipfs_gemm_workspace_floats(int M, int N, int K) { return shape_query(M, N, K).workspace_floats; }
extern "C" size_t clipfs_gemm_counter_ints(int M, int N, int K) { return shape_query(M, N, K).counter_ints; }

extern "C" int clipfs_gemm_timing(int enable) {
  g_timing = enable != 0;
  return CLIPFS_OK;
}

extern "C" double clipfs_gemm_timing_last_bytes(void) { return g_last_bytes; }

extern "C" int clipfs_gemm_timing_collect(double* total_ms, double* total_flops, int* launches) {
  double ms = 0.0, fl = 0.0, by = 0.0;
  int n = 0;
  if (g_timed) {
    for (TimedLaunch& t : *g_timed) {
      float e = 0.f;
      if (hipEventSynchronize(t.stop) == hipSuccess && hipEventElapsedTime(&e, t.start, t.stop) == hipSuccess) {
        ms += e;
        fl += t.flops;
        by += t.bytes;
        ++n;
      }
      (void)hipEventDestroy(t.start);
      (void)hipEventDestroy(t.stop);
    }
    g_timed->clear();
  }
  g_last_bytes = by;
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  if (launches) *launches = n;
  return CLIPFS_OK;
}

namespace clipfs {
int gemm_bf16x3_dispatch(const GemmParams& base, const GemmPlan& plan, hipStream_t stream);  // gemm_bf16.hip
int gemm_f16_dispatch(const clipfs_gemm_args& a, hipStream_t stream);  // gemm_f16.hip
void gemm_f16_plan(const clipfs_gemm_args& a, int cus, clipfs_f16_plan* out);
}

static int gemm_nt_impl(const clipfs_gemm_args* args, void* stream);

// what the f16 x f16 kernel requires of its arguments (shared by clipfs_gemm_nt and clipfs_gemm_f16_plan)
static int gemm_f16_validate(const clipfs_gemm_args& a) {
  CLIPFS_REQUIRE(a.B_planes && a.b_format == 2, "gemm: A_f16 needs the f16 copy of B (b_format 2)");
  CLIPFS_REQUIRE(a.C || a.C_f16, "gemm: no output");
  CLIPFS_REQUIRE(a.a_mode == 0 && (a.K % BK) == 0 && (a.lda & 7) == 0 && (a.ldb & 7) == 0 && a.lda >= a.K && a.ldb >= a.K &&
                     a.ldc >= a.N && aligned16(a.A_f16) && aligned16(a.B_planes),
                 "gemm f16: K %% 32, lda/ldb %% 8, 16-byte aligned operands required");
  CLIPFS_REQUIRE(a.act >= 0 && a.act <= 2 && (a.act != 2 || a.aux_in) && (!a.residual || a.ldres >= a.N), "gemm f16: bad epilogue args");
  if (a.lora_t) {
    CLIPFS_REQUIRE(a.lora_b && a.lora_r > 0 && a.lora_r <= 64 && a.lora_nseg > 0 && a.lora_seg_width % 128 == 0 &&
                       a.lora_seg_width * a.lora_nseg >= a.N, "gemm f16: lora rank <= 64 and segment width %% 128 required");
    // the adapter product is accumulated by MFMA steps into the same accumulator that alpha then scales
    CLIPFS_REQUIRE(a.alpha == 1.f, "gemm f16: alpha != 1 (%g) together with lora_t is not supported: alpha would scale the adapter term",
                   (double)a.alpha);
  }
  return CLIPFS_OK;
}

extern "C" int clipfs_gemm_f16_plan(const clipfs_gemm_args* args, int cus, clipfs_f16_plan* out) {
  CLIPFS_REQUIRE(args != nullptr && out != nullptr, "gemm f16 plan: null args / out");
  const clipfs_gemm_args& a = *args;
  CLIPFS_REQUIRE(a.struct_size == sizeof(clipfs_gemm_args),
                 "gemm f16 plan: args built against another clipfs.h (struct_size %zu, library has %zu)", a.struct_size,
                 sizeof(clipfs_gemm_args));
  CLIPFS_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm f16 plan: bad dims %d %d %d", a.M, a.N, a.K);
  CLIPFS_REQUIRE(a.A_f16 != nullptr, "gemm f16 plan: A_f16 is not set (the plan is that of the f16 x f16 kernel)");
  CLIPFS_CHECK(gemm_f16_validate(a));
  clipfs::gemm_f16_plan(a, cus, out);
  return CLIPFS_OK;
}

extern "C" int clipfs_gemm_nt(const clipfs_gemm_args* args, void* stream) {
  if (!g_timing) return gemm_nt_impl(args, stream);
  TimedLaunch tl;
  (void)hipEventCreate(&tl.start);
  (void)hipEventCreate(&tl.stop);
  tl.flops = args ? 2.0 * args->M * (double)args->N * args->K : 0.0;
  tl.bytes = 0.0;
  if (args) {
    const double mk = (double)args->M * args->K, nk = (double)args->N * args->K, mn = (double)args->M * args->N;
    const double ab = args->A_f16 ? 2.0 : 4.0, bb = args->B_planes ? (args->b_format == 1 ? 4.0 : 2.0) : 4.0;
    tl.bytes = ab * mk + bb * nk + (args->C ? 4.0 : 0.0) * mn + (args->C_f16 ? 2.0 : 0.0) * mn +
               4.0 * mn * ((args->residual ? 1 : 0) + (args->aux_out && args->act == 1 ? 1 : 0) + (args->act == 2 ? 1 : 0));
  }
  (void)hipEventRecord(tl.start, (hipStream_t)stream);
  const int rc = gemm_nt_impl(args, stream);
  (void)hipEventRecord(tl.stop, (hipStream_t)stream);
  if (!g_timed) g_timed = new std::vector<TimedLaunch>();
  g_timed->push_back(tl);
  return rc;
}

// what every clipfs_gemm_nt call must satisfy before its kernel family is looked at
static int gemm_validate_head(const clipfs_gemm_args* args) {
  CLIPFS_REQUIRE(args != nullptr, "gemm: null args");
  const clipfs_gemm_args& a = *args;
  CLIPFS_REQUIRE(a.struct_size == sizeof(clipfs_gemm_args),
                 "gemm: args built against another clipfs.h (struct_size %zu, library has %zu)", a.struct_size,
                 sizeof(clipfs_gemm_args));
  CLIPFS_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm: bad dims %d %d %d", a.M, a.N, a.K);
  return CLIPFS_OK;
}

// what the exact fp32 and the 16-bit-plane kernels require (shared by clipfs_gemm_nt and clipfs_gemm_plan)
static int gemm_validate(const clipfs_gemm_args& a) {
  CLIPFS_REQUIRE(!a.C_f16 && !a.aux_f16, "gemm: C_f16 / aux_f16 belong to the f16 x f16 kernel only");
  CLIPFS_REQUIRE(a.A && a.B && a.C, "gemm: null operand");
  CLIPFS_REQUIRE((a.K & 3) == 0 && (a.ldb & 3) == 0 && aligned16(a.B), "gemm: K and ldb must be multiples of 4, B 16-byte aligned");
  CLIPFS_REQUIRE(a.ldb >= a.K && a.ldc >= a.N, "gemm: leading dimension too small");
  CLIPFS_REQUIRE(a.act >= 0 && a.act <= 3, "gemm: bad act %d", a.act);
  CLIPFS_REQUIRE(a.act != 3 || !a.B_planes, "gemm: act 3 (ReLU) belongs to the exact fp32 kernels");
  CLIPFS_REQUIRE(a.act != 2 || a.aux_in, "gemm: act 2 needs aux_in");
  CLIPFS_REQUIRE(!a.residual || a.ldres >= a.N, "gemm: ldres too small");
  if (a.a_mode == 0) {
    CLIPFS_REQUIRE((a.lda & 3) == 0 && a.lda >= a.K && aligned16(a.A), "gemm: lda must be a multiple of 4 and >= K, A 16-byte aligned");
  } else {
    CLIPFS_REQUIRE(a.a_mode == 1, "gemm: bad a_mode %d", a.a_mode);
    CLIPFS_REQUIRE(a.patch > 0 && a.img_res % a.patch == 0, "gemm: image %d not divisible by patch %d", a.img_res, a.patch);
    const int patches = (a.img_res / a.patch) * (a.img_res / a.patch);
    CLIPFS_REQUIRE(a.K == 3 * a.patch * a.patch, "gemm: patch mode needs K == 3*patch^2");
    CLIPFS_REQUIRE(a.M % patches == 0 && a.out_tokens >= patches + 1, "gemm: patch mode shape mismatch");
    CLIPFS_REQUIRE((a.patch & 3) != 0 || ((a.img_res & 3) == 0 && aligned16(a.A)), "gemm: image rows must be 16-byte aligned");
  }
  if (a.lora_t) {
    CLIPFS_REQUIRE(a.lora_b && a.lora_r > 0 && a.lora_nseg > 0 && a.lora_seg_width > 0, "gemm: bad lora args");
    CLIPFS_REQUIRE(a.lora_seg_width % 32 == 0 && a.lora_seg_width * a.lora_nseg >= a.N, "gemm: lora segment width must be a multiple of 32 and cover N");
  }
  return CLIPFS_OK;
}

// the route of validated arguments, and its schedule with the scratch as given
static GemmSchedule gemm_schedule_of(const clipfs_gemm_args& a) {
  static const int glds_cfg = env_int("CLIPFS_GEMM_GLDS", 1);  // 0: register staging (A/B aid)
  const bool dense32 = a.a_mode == 0 && (a.K % BK) == 0;
  const GemmRoute route = dense32 && a.B_planes && (a.b_format == 1 || a.b_format == 2) && a.ldb == a.K ? ROUTE_PLANES
                          : dense32 ? ROUTE_DENSE
                          : a.a_mode == 1 && a.patch == 32 && (a.img_res & 3) == 0 ? ROUTE_PATCH32 : ROUTE_GENERIC;
  return gemm_schedule(a.M, a.N, a.K, route, a.b_format == 2 ? 1 : 2, glds_cfg != 0, &a);
}

extern "C" int clipfs_gemm_plan(const clipfs_gemm_args* args, struct clipfs_gemm_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "gemm plan: null plan");
  CLIPFS_CHECK(gemm_validate_head(args));
  CLIPFS_REQUIRE(!args->A_f16, "gemm plan: A_f16 is set: the f16 x f16 kernel's plan is clipfs_gemm_f16_plan");
  CLIPFS_CHECK(gemm_validate(*args));
  *plan = gemm_schedule_of(*args).plan;
  return CLIPFS_OK;
}

template <void (*KERNEL)(const GemmParams)>
static int launch(const GemmPlan& plan, const GemmParams& p, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set && plan.lds_bytes > 48 * 1024) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, plan.lds_bytes);
    attr_set = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, p);
  return launch_status();
}

static int gemm_nt_impl(const clipfs_gemm_args* args, void* stream) {
  CLIPFS_CHECK(gemm_validate_head(args));
  const clipfs_gemm_args& a = *args;
  if (a.A_f16) {  // f16 x f16 kernel
    CLIPFS_CHECK(gemm_f16_validate(a));
    return gemm_f16_dispatch(a, (hipStream_t)stream);
  }
  CLIPFS_CHECK(gemm_validate(a));
  const GemmSchedule sc = gemm_schedule_of(a);
  const GemmPlan& plan = sc.plan;
  GemmParams p;
  p.a = a;
  p.n_blocks_n = sc.n_blocks_n;
  p.grid_g = a.a_mode == 1 ? a.img_res / a.patch : 0;
  p.patches = p.grid_g * p.grid_g;
  p.splits = plan.splits;
  p.part = plan.splits > 1 ? a.workspace : nullptr;
  p.cnt = plan.splits > 1 ? a.counters : nullptr;
  p.gm = plan.gm;
#ifdef CLIPFS_ABLATION_BUILD
  static const int ablate_cfg = env_int("CLIPFS_GEMM_ABLATE", 0);
  p.ablate = ablate_cfg;
#else
  p.ablate = 0;
#endif
  p.mix_rows64 = plan.mix_rows64;
  p.mix_tiles64 = sc.mix_tiles64;
  hipStream_t s = (hipStream_t)stream;
  switch (plan.kernel) {
    case CLIPFS_GEMM_NT64: return launch<gemm_nt_kernel<64, 128, 3>>(plan, p, s);
    case CLIPFS_GEMM_NT64_REG: return launch<gemm_nt_kernel<64, 128, 0>>(plan, p, s);
    case CLIPFS_GEMM_NT32: return launch<gemm_nt_kernel<32, 128, 3>>(plan, p, s);
    case CLIPFS_GEMM_MIXED: return launch<gemm_nt_mixed_kernel>(plan, p, s);
    case CLIPFS_GEMM_PATCH32: return launch<gemm_nt_kernel<64, 128, 1>>(plan, p, s);
    case CLIPFS_GEMM_GENERIC: return launch<gemm_nt_kernel<64, 128, 2>>(plan, p, s);
    default: return gemm_bf16x3_dispatch(p, plan, s);  // CLIPFS_GEMM_PLANES64 / _PLANES128
  }
}

