// Training-free dynamic adapter (clipfs.h "TDA"; Karmanov et al., CVPR 2024), fp32 in every engine precision mode: a
// zero-shot classifier adapted by two device-resident test-time caches, a whole batch per call, EXACTLY the sequential
// one-sample-at-a-time rule of the header.
//
// The insertions of a sample depend only on (pred, H, h) of the samples before it and never on a cache logit, and the
// queues of different classes are independent.  So the sequential rule becomes intervals: entry j (an old slot or a batch
// row) is in the cache for the queries born_j <= i < evict_j of the batch, and the logits are a dense masked sum.
//
//   z      one workgroup per (32 classes, 32 rows): out = s F T^T on v_mfma_f32_32x32x2_f32 (tile_dots of logits_tile.h,
//          the four waves splitting the 64-feature steps, partials added in wave order).  Every element sums the same
//          features in the same order wherever its row sits.
//   stats  one wave per row: max, argmax (ties to the lower class), sum of exponentials, H = log(sum) - sum(e t) / sum
//          with t = z - max, h = H / log2 C, the band flag and the mask row.  Lane l takes classes l, l + 64, ...; the
//          wave sums are DPP butterflies: a row's numbers do not depend on B or on the row index.
//   scan   one thread per class walks the batch's (pred, H, band) in row order (staged through LDS 1024 rows at a time)
//          with its two queues in registers and writes born / evict of every old slot and batch row and the slot of every
//          inserted row.  No feature is touched.
//   logits one workgroup per (32 rows, 256 classes) walks four entry segments in this order: positive old slots,
//          positive batch rows, negative old slots, negative batch rows; each in tiles of 32 entries ascending.  A tile
//          none of whose entries is live for the workgroup's rows (or, positive cache, of its classes) is skipped.  For a
//          live tile the 32 x 32 affinities are formed as in the z kernel, G = +pos_alpha E or -neg_alpha E inside the
//          interval and 0 outside, and every wave contracts G with the tile's value rows (one-hot class for the positive
//          cache, mask bytes for the negative one) into its 64 classes on the matrix cores: step i of 16 adds entries i
//          and 16 + i of the tile.  At the end out = z + sum, one thread per element.  The affinities never reach memory.
//   write  one workgroup per batch row: a row that was inserted and is still in its queue at the end of the batch
//          (evict == B) is copied into its slot with its entropy, sequence number and mask row; the counter advances.
//
// No float atomics; every output element is written by one thread; every sum runs in the order given above, fixed by the
// shapes, the state layout and the intervals.  Nothing returns to the host.
#include "logits_tile.h"

#include <math.h>

namespace clipfs {
namespace {

constexpr int TDA_THREADS = 256;
constexpr int TDA_MAX_S = 8;        // slots per queue
constexpr int TDA_SCAN_T = 64;      // classes (threads) per scan workgroup
constexpr int TDA_SCAN_ROWS = 1024; // batch rows staged per pass of the scan
constexpr int TDA_NACC = 2;         // 32-class accumulators per wave of the logits kernel
constexpr int TDA_CC = 4 * 32 * TDA_NACC;  // classes per logits workgroup

__device__ __forceinline__ float tda_exp(float a, float bl2) { return __builtin_amdgcn_exp2f((a - 1.f) * bl2); }

// ------------------------------------------------------------------------------------------------- z
__global__ __launch_bounds__(TDA_THREADS) void tda_z_kernel(const float* __restrict__ F, const float* __restrict__ T,
                                                            float* __restrict__ out, int B, int C, int d, int ldo, float s) {
  __shared__ float Ps[4][32 * TILE_PS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int c0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const f32x16 acc = tile_dots(F, b0, B, T, c0, C, d, 64 * w, 256, lane);
#pragma unroll
  for (int r = 0; r < 16; ++r) Ps[w][tile_row(r, h) * TILE_PS + li] = acc[r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + TDA_THREADS * i, row = e >> 5, col = e & 31;
    const float a = tile_sum4(Ps, row * TILE_PS + col);
    if (b0 + row < B && c0 + col < C) out[(size_t)(b0 + row) * ldo + c0 + col] = s * a;
  }
}

// ------------------------------------------------------------------------------------------------- stats
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(TDA_THREADS) void tda_stats_kernel(const float* __restrict__ out, int ldo, int32_t* __restrict__ pred,
                                                                float* __restrict__ ent, float* __restrict__ hnorm,
                                                                int32_t* __restrict__ band, uint8_t* __restrict__ mask, int B,
                                                                int C, float ent_lo, float ent_hi, float mask_lo,
                                                                float mask_hi) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * (TDA_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform; no barrier in this kernel
  const float* zr = out + (size_t)b * ldo;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, zr[c]);
  m = wave_max(m);
  int best = C;
  for (int c = lane; c < C; c += 64)
    if (zr[c] == m && c < best) best = c;
  best = wave_min_int(best);
  if (best >= C) best = 0;  // a row that is not numbers: class 0
  float ssum = 0.f, a = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float t = zr[c] - m, e = expf(t);
    ssum += e;
    a += e * t;
  }
  ssum = wave_sum(ssum);
  a = wave_sum(a);
  const float H = logf(ssum) - a / ssum;
  const float hn = C > 1 ? H / log2f((float)C) : 0.f;
  for (int c = lane; c < C; c += 64) {
    const float p = expf(zr[c] - m) / ssum;
    mask[(size_t)b * C + c] = (mask_lo < p && p < mask_hi) ? 1 : 0;
  }
  if (lane == 0) {
    pred[b] = best;
    ent[b] = H;
    hnorm[b] = hn;
    band[b] = (ent_lo < hn && hn < ent_hi) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------- scan
// One queue of one class, in registers (every index is a compile-time constant after unrolling).  born / evict are indexed
// by entry: old slot (c, k) is entry c * S + k, batch row b entry C * S + b.
struct TdaQueue {
  float ent[TDA_MAX_S];
  long long seq[TDA_MAX_S];
  int owner[TDA_MAX_S], born[TDA_MAX_S];
  __device__ __forceinline__ void load(const float* __restrict__ s_ent, const long long* __restrict__ s_seq, int c, int S) {
#pragma unroll
    for (int k = 0; k < TDA_MAX_S; ++k) {
      const bool in = k < S;
      ent[k] = in ? s_ent[(size_t)c * S + k] : INFINITY;
      seq[k] = in ? s_seq[(size_t)c * S + k] : -1;
      owner[k] = c * S + k;
      born[k] = 0;
    }
  }
  // the rule's step 7 for entropy H at batch row b, sample number t; returns the slot or -1
  __device__ __forceinline__ int offer(float H, long long t, int b, int entry, int S, int32_t* __restrict__ g_born,
                                       int32_t* __restrict__ g_evict) {
    int slot = -1;
#pragma unroll
    for (int k = TDA_MAX_S - 1; k >= 0; --k)
      if (k < S && seq[k] < 0) slot = k;  // the lowest free slot
    if (slot < 0) {
      int w = 0, ow = owner[0], bw = born[0];
      float ew = ent[0];
      long long sw = seq[0];
#pragma unroll
      for (int k = 1; k < TDA_MAX_S; ++k)
        if (k < S && (ent[k] > ew || (ent[k] == ew && seq[k] > sw))) {  // largest entropy, ties to the latest
          w = k;
          ew = ent[k];
          sw = seq[k];
          ow = owner[k];  // carried along: indexing by w afterwards would keep the record out of registers
          bw = born[k];
        }
      if (H < ew) {
        slot = w;
        g_born[ow] = bw;  // the loser's interval closes here: row b no longer sees it
        g_evict[ow] = b;
      }
    }
    if (slot >= 0) {
#pragma unroll
      for (int k = 0; k < TDA_MAX_S; ++k)
        if (k == slot) {
          ent[k] = H;
          seq[k] = t;
          owner[k] = entry;
          born[k] = b;
        }
    } else {
      g_born[entry] = 0;
      g_evict[entry] = 0;
    }
    return slot;
  }
  // an old slot that is empty is never in the cache: written at once, because a batch row that takes the slot takes over
  // owner[k], and the old entry's interval would otherwise stay unwritten
  __device__ __forceinline__ void start(int S, int32_t* __restrict__ g_born, int32_t* __restrict__ g_evict) const {
#pragma unroll
    for (int k = 0; k < TDA_MAX_S; ++k)
      if (k < S && seq[k] < 0) {
        g_born[owner[k]] = 0;
        g_evict[owner[k]] = 0;
      }
  }
  // the survivors live to the end of the batch; a slot that stayed empty gets the empty interval
  __device__ __forceinline__ void finish(int S, int B, int32_t* __restrict__ g_born, int32_t* __restrict__ g_evict) const {
#pragma unroll
    for (int k = 0; k < TDA_MAX_S; ++k)
      if (k < S) {
        g_born[owner[k]] = seq[k] >= 0 ? born[k] : 0;
        g_evict[owner[k]] = seq[k] >= 0 ? B : 0;
      }
  }
};

__global__ __launch_bounds__(TDA_SCAN_T) void tda_scan_kernel(const int32_t* __restrict__ pred, const float* __restrict__ ent,
                                                              const int32_t* __restrict__ band, const float* __restrict__ pos_ent,
                                                              const long long* __restrict__ pos_seq,
                                                              const float* __restrict__ neg_ent,
                                                              const long long* __restrict__ neg_seq,
                                                              const long long* __restrict__ counter, long long* __restrict__ seq,
                                                              int32_t* __restrict__ pos_slot, int32_t* __restrict__ neg_slot,
                                                              int32_t* __restrict__ pos_born, int32_t* __restrict__ pos_evict,
                                                              int32_t* __restrict__ neg_born, int32_t* __restrict__ neg_evict,
                                                              int B, int C, int Sp, int Sn, int update) {
  __shared__ int s_pred[TDA_SCAN_ROWS], s_band[TDA_SCAN_ROWS];
  __shared__ float s_H[TDA_SCAN_ROWS];
  const int tid = threadIdx.x, c = blockIdx.x * TDA_SCAN_T + tid;
  const bool own = c < C;
  const long long t0 = counter[0];
  TdaQueue qp, qn;
  if (own) {
    qp.load(pos_ent, pos_seq, c, Sp);
    qn.load(neg_ent, neg_seq, c, Sn);
    qp.start(Sp, pos_born, pos_evict);
    qn.start(Sn, neg_born, neg_evict);
  }
  for (int r0 = 0; r0 < B; r0 += TDA_SCAN_ROWS) {
    const int n = min(TDA_SCAN_ROWS, B - r0);
    __syncthreads();
    for (int i = tid; i < n; i += TDA_SCAN_T) {
      s_pred[i] = pred[r0 + i];
      s_band[i] = band[r0 + i];
      s_H[i] = ent[r0 + i];
    }
    __syncthreads();
    if (!own) continue;
    for (int i = 0; i < n; ++i) {
      if (s_pred[i] != c) continue;
      const int b = r0 + i;
      const float H = s_H[i];
      seq[b] = t0 + b;
      int sp = -1, sn = -1;
      if (update && Sp > 0) sp = qp.offer(H, t0 + b, b, C * Sp + b, Sp, pos_born, pos_evict);
      else {
        pos_born[C * Sp + b] = 0;
        pos_evict[C * Sp + b] = 0;
      }
      if (update && Sn > 0 && s_band[i]) sn = qn.offer(H, t0 + b, b, C * Sn + b, Sn, neg_born, neg_evict);
      else {
        neg_born[C * Sn + b] = 0;
        neg_evict[C * Sn + b] = 0;
      }
      pos_slot[b] = sp;
      neg_slot[b] = sn;
    }
  }
  if (own) {
    qp.finish(Sp, B, pos_born, pos_evict);
    qn.finish(Sn, B, neg_born, neg_evict);
  }
}

// ------------------------------------------------------------------------------------------------- logits
struct TdaSegment {
  const float* keys;       // [n, d]
  const int32_t* born;     // [n] (already offset to the segment)
  const int32_t* evict;
  const int32_t* cls;      // positive batch rows: pred; NULL: entry / S
  const uint8_t* values;   // negative: mask rows [n, C]; NULL: one-hot class
  int n, S;
  float g, bl2;            // +pos_alpha / -neg_alpha, beta log2(e)
};

__global__ __launch_bounds__(TDA_THREADS) void tda_logits_kernel(const float* __restrict__ F, TdaSegment g0, TdaSegment g1,
                                                                 TdaSegment g2, TdaSegment g3, float* __restrict__ out, int B,
                                                                 int C, int d, int ldo) {
  __shared__ float Ps[4][32 * TILE_PS];  // per wave: [row][entry] partial dot products over its 64-feature steps
  __shared__ float Gs[32 * 32];          // [entry][row]
  __shared__ int s_born[32], s_evict[32], s_cls[32];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * 32, c0 = blockIdx.y * TDA_CC, c1 = min(C, c0 + TDA_CC);
  const int cw = c0 + w * 32 * TDA_NACC;  // this wave's first class
  f32x16 acc[TDA_NACC];
#pragma unroll
  for (int a = 0; a < TDA_NACC; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
  const int xlast = min(x0 + 32, B);  // rows [x0, xlast)
  for (int sgi = 0; sgi < 4; ++sgi) {
    const TdaSegment sg = sgi == 0 ? g0 : sgi == 1 ? g1 : sgi == 2 ? g2 : g3;
    for (int y0 = 0; y0 < sg.n; y0 += 32) {
      __syncthreads();  // the last tile's readers of s_* and Gs are done
      int live = 0;
      if (tid < 32) {
        const int y = y0 + tid;
        int bo = 0, ev = 0, cl = -1;
        if (y < sg.n) {
          bo = sg.born[y];
          ev = sg.evict[y];
          cl = sg.values ? -1 : (sg.cls ? sg.cls[y] : y / sg.S);
          live = bo < xlast && ev > x0 && ev > bo && (sg.values || (cl >= c0 && cl < c1));
        }
        s_born[tid] = bo;
        s_evict[tid] = ev;
        s_cls[tid] = cl;
      }
      if (!__syncthreads_or(live)) continue;  // workgroup-uniform
      const f32x16 s = tile_dots(F, x0, B, sg.keys, y0, sg.n, d, 64 * w, 256, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) Ps[w][tile_row(r, h) * TILE_PS + li] = s[r];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = tid + TDA_THREADS * i, own = e & 31, oth = e >> 5;
        const float a = tile_sum4(Ps, own * TILE_PS + oth);
        const int xi = x0 + own;
        float g = 0.f;
        if (xi < B && s_born[oth] <= xi && xi < s_evict[oth]) g = sg.g * tda_exp(a, sg.bl2);
        Gs[oth * 32 + own] = g;
      }
      __syncthreads();
      float ga[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) ga[i] = Gs[(16 * h + i) * 32 + li];
#pragma unroll
      for (int a = 0; a < TDA_NACC; ++a) {
        if (cw + 32 * a < c1) {  // wave-uniform
          const int ct = cw + 32 * a + li;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int oth = 16 * h + i, y = min(y0 + oth, sg.n - 1);
            float v;
            if (sg.values) v = ct < C ? (float)sg.values[(size_t)y * C + ct] : 0.f;
            else v = s_cls[oth] == ct ? 1.f : 0.f;
            acc[a] = tile_mfma(ga[i], v, acc[a]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < TDA_NACC; ++a) {
    const int ct = cw + 32 * a + li;
    if (ct < C) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int xi = x0 + tile_row(r, h);
        if (xi < B) {
          float* p = out + (size_t)xi * ldo + ct;
          *p = *p + acc[a][r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- write-back
__global__ __launch_bounds__(TDA_THREADS) void tda_write_kernel(const float* __restrict__ F, const int32_t* __restrict__ pred,
                                                                const float* __restrict__ ent, const long long* __restrict__ seq,
                                                                const uint8_t* __restrict__ mask,
                                                                const int32_t* __restrict__ pos_slot,
                                                                const int32_t* __restrict__ neg_slot,
                                                                const int32_t* __restrict__ pos_evict,
                                                                const int32_t* __restrict__ neg_evict, float* __restrict__ pos_keys,
                                                                float* __restrict__ pos_ent, long long* __restrict__ pos_seq,
                                                                float* __restrict__ neg_keys, float* __restrict__ neg_ent,
                                                                long long* __restrict__ neg_seq, uint8_t* __restrict__ neg_mask,
                                                                long long* __restrict__ counter, int B, int C, int d, int Sp,
                                                                int Sn) {
  const int tid = threadIdx.x, b = blockIdx.x;
  const int c = pred[b];
  const f32x4* src = reinterpret_cast<const f32x4*>(F + (size_t)b * d);
  const int sp = pos_slot[b], sn = neg_slot[b];
  if (sp >= 0 && sp < Sp && c >= 0 && c < C && pos_evict[C * Sp + b] == B) {
    const size_t at = (size_t)c * Sp + sp;
    f32x4* dst = reinterpret_cast<f32x4*>(pos_keys + at * d);
    for (int j = tid; j < d / 4; j += TDA_THREADS) dst[j] = src[j];
    if (tid == 0) {
      pos_ent[at] = ent[b];
      pos_seq[at] = seq[b];
    }
  }
  if (sn >= 0 && sn < Sn && c >= 0 && c < C && neg_evict[C * Sn + b] == B) {
    const size_t at = (size_t)c * Sn + sn;
    f32x4* dst = reinterpret_cast<f32x4*>(neg_keys + at * d);
    for (int j = tid; j < d / 4; j += TDA_THREADS) dst[j] = src[j];
    for (int j = tid; j < C; j += TDA_THREADS) neg_mask[at * C + j] = mask[(size_t)b * C + j];
    if (tid == 0) {
      neg_ent[at] = ent[b];
      neg_seq[at] = seq[b];
    }
  }
  if (b == 0 && tid == 0) counter[0] = counter[0] + B;  // read by the scan alone, which ran before this launch
}

int tda_check_params(const struct clipfs_tda_params* p, const char* who) {
  CLIPFS_REQUIRE(p != nullptr, "%s: NULL params", who);
  CLIPFS_REQUIRE(p->struct_size == sizeof(struct clipfs_tda_params), "%s: params.struct_size = %u, this library expects %u",
                 who, p->struct_size, (unsigned)sizeof(struct clipfs_tda_params));
  CLIPFS_REQUIRE(p->d >= 4 && p->d <= 4096 && p->d % 4 == 0, "%s: d = %d must be a multiple of 4 in [4, 4096]", who, p->d);
  CLIPFS_REQUIRE(p->C >= 1 && p->C <= 4096, "%s: C = %d outside [1, 4096]", who, p->C);
  CLIPFS_REQUIRE(p->pos_cap >= 0 && p->pos_cap <= TDA_MAX_S, "%s: pos_cap = %d outside [0, %d]", who, p->pos_cap, TDA_MAX_S);
  CLIPFS_REQUIRE(p->neg_cap >= 0 && p->neg_cap <= TDA_MAX_S, "%s: neg_cap = %d outside [0, %d]", who, p->neg_cap, TDA_MAX_S);
  CLIPFS_REQUIRE(isfinite(p->logit_scale), "%s: logit_scale is not finite", who);
  CLIPFS_REQUIRE(isfinite(p->pos_alpha) && p->pos_alpha >= 0.f, "%s: pos_alpha = %g must be finite and >= 0", who,
                 (double)p->pos_alpha);
  CLIPFS_REQUIRE(isfinite(p->pos_beta) && p->pos_beta >= 0.f, "%s: pos_beta = %g must be finite and >= 0", who,
                 (double)p->pos_beta);
  CLIPFS_REQUIRE(isfinite(p->neg_alpha) && p->neg_alpha >= 0.f, "%s: neg_alpha = %g must be finite and >= 0", who,
                 (double)p->neg_alpha);
  CLIPFS_REQUIRE(isfinite(p->neg_beta) && p->neg_beta >= 0.f, "%s: neg_beta = %g must be finite and >= 0", who,
                 (double)p->neg_beta);
  CLIPFS_REQUIRE(!isnan(p->ent_lo) && !isnan(p->ent_hi) && !isnan(p->mask_lo) && !isnan(p->mask_hi),
                 "%s: ent_lo / ent_hi / mask_lo / mask_hi is not a number", who);
  return CLIPFS_OK;
}

bool tda_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_tda_plan(const struct clipfs_tda_params* params, int B, int update, struct clipfs_tda_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_tda_plan: NULL plan");
  CLIPFS_CHECK(tda_check_params(params, "clipfs_tda_plan"));
  CLIPFS_REQUIRE(B >= 1 && B <= 8192, "clipfs_tda_plan: B = %d outside [1, 8192]", B);
  const int C = params->C, d = params->d, Sp = params->pos_cap, Sn = params->neg_cap;
  struct clipfs_tda_plan p = {};
  const unsigned qt = (unsigned)((B + 31) / 32);
  const unsigned tile_lds = (unsigned)(4 * 32 * TILE_PS * sizeof(float));
  p.launch[CLIPFS_TDA_LAUNCH_Z] = {(unsigned)((C + 31) / 32), qt, TDA_THREADS, tile_lds};
  p.launch[CLIPFS_TDA_LAUNCH_STATS] = {(unsigned)((B + 3) / 4), 1, TDA_THREADS, 0};
  p.launch[CLIPFS_TDA_LAUNCH_SCAN] = {(unsigned)((C + TDA_SCAN_T - 1) / TDA_SCAN_T), 1, TDA_SCAN_T,
                                      (unsigned)(3 * TDA_SCAN_ROWS * sizeof(float))};
  if (Sp > 0 || Sn > 0)
    p.launch[CLIPFS_TDA_LAUNCH_LOGITS] = {qt, (unsigned)((C + TDA_CC - 1) / TDA_CC), TDA_THREADS,
                                          (unsigned)(tile_lds + (32 * 32 + 3 * 32) * sizeof(float))};
  if (update) p.launch[CLIPFS_TDA_LAUNCH_WRITE] = {(unsigned)B, 1, TDA_THREADS, 0};
  for (int i = 0; i < CLIPFS_TDA_LAUNCHES; ++i) {
    if (p.launch[i].grid_x) ++p.launches;
    if (p.launch[i].lds_bytes > p.lds_bytes) p.lds_bytes = p.launch[i].lds_bytes;
  }
  p.class_chunk = TDA_CC;
  p.pos_entries = (size_t)C * Sp + B;
  p.neg_entries = (size_t)C * Sn + B;
  p.pos_key_floats = (size_t)C * Sp * d;
  p.neg_key_floats = (size_t)C * Sn * d;
  p.neg_mask_bytes = (size_t)C * Sn * C;
  p.mask_bytes = (size_t)B * C;
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_tda_adapt(const struct clipfs_tda_params* params, const float* feats, const float* text,
                                const struct clipfs_tda_state* state, float* out, int ldout,
                                const struct clipfs_tda_record* record, int B, int update, void* stream) {
  struct clipfs_tda_plan p;
  CLIPFS_CHECK(clipfs_tda_plan(params, B, update, &p));
  const int C = params->C, d = params->d, Sp = params->pos_cap, Sn = params->neg_cap;
  CLIPFS_REQUIRE(feats && aligned16(feats), "clipfs_tda_adapt: feats is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(text && aligned16(text), "clipfs_tda_adapt: text is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(out && aligned16(out), "clipfs_tda_adapt: out is NULL or not 16-byte aligned");
  CLIPFS_REQUIRE(ldout >= C, "clipfs_tda_adapt: ldout = %d below C = %d", ldout, C);
  CLIPFS_REQUIRE(state != nullptr, "clipfs_tda_adapt: NULL state");
  CLIPFS_REQUIRE(state->struct_size == sizeof(struct clipfs_tda_state), "clipfs_tda_adapt: state.struct_size = %u, expected %u",
                 state->struct_size, (unsigned)sizeof(struct clipfs_tda_state));
  CLIPFS_REQUIRE(record != nullptr, "clipfs_tda_adapt: NULL record");
  CLIPFS_REQUIRE(record->struct_size == sizeof(struct clipfs_tda_record),
                 "clipfs_tda_adapt: record.struct_size = %u, expected %u", record->struct_size,
                 (unsigned)sizeof(struct clipfs_tda_record));
  CLIPFS_REQUIRE(state->counter, "clipfs_tda_adapt: state.counter is NULL");
  if (Sp > 0) {
    CLIPFS_REQUIRE(state->pos_keys && aligned16(state->pos_keys), "clipfs_tda_adapt: state.pos_keys is NULL or not 16-byte aligned");
    CLIPFS_REQUIRE(state->pos_ent && state->pos_seq, "clipfs_tda_adapt: state.pos_ent or state.pos_seq is NULL");
  }
  if (Sn > 0) {
    CLIPFS_REQUIRE(state->neg_keys && aligned16(state->neg_keys), "clipfs_tda_adapt: state.neg_keys is NULL or not 16-byte aligned");
    CLIPFS_REQUIRE(state->neg_ent && state->neg_seq && state->neg_mask,
                   "clipfs_tda_adapt: state.neg_ent, state.neg_seq or state.neg_mask is NULL");
  }
  CLIPFS_REQUIRE(record->pred && record->entropy && record->hnorm && record->band && record->seq && record->mask &&
                     record->pos_slot && record->neg_slot && record->pos_born && record->pos_evict && record->neg_born &&
                     record->neg_evict,
                 "clipfs_tda_adapt: a member of record is NULL (all twelve arrays are written)");
  const size_t out_bytes = ((size_t)(B - 1) * ldout + C) * sizeof(float);
  CLIPFS_REQUIRE(!tda_overlap(out, out_bytes, feats, (size_t)B * d * 4) && !tda_overlap(out, out_bytes, text, (size_t)C * d * 4) &&
                     !tda_overlap(out, out_bytes, state->pos_keys, p.pos_key_floats * 4) &&
                     !tda_overlap(out, out_bytes, state->neg_keys, p.neg_key_floats * 4),
                 "clipfs_tda_adapt: out aliases feats, text or a key tensor of state");
  hipStream_t st = (hipStream_t)stream;
  const struct clipfs_tda_launch* L = p.launch;
  hipLaunchKernelGGL(tda_z_kernel, dim3(L[0].grid_x, L[0].grid_y), dim3(L[0].block), 0, st, feats, text, out, B, C, d, ldout,
                     params->logit_scale);
  hipLaunchKernelGGL(tda_stats_kernel, dim3(L[1].grid_x), dim3(L[1].block), 0, st, out, ldout, record->pred, record->entropy,
                     record->hnorm, record->band, record->mask, B, C, params->ent_lo, params->ent_hi, params->mask_lo,
                     params->mask_hi);
  hipLaunchKernelGGL(tda_scan_kernel, dim3(L[2].grid_x), dim3(L[2].block), 0, st, record->pred, record->entropy, record->band,
                     state->pos_ent, (const long long*)state->pos_seq, state->neg_ent, (const long long*)state->neg_seq,
                     (const long long*)state->counter, (long long*)record->seq, record->pos_slot, record->neg_slot,
                     record->pos_born, record->pos_evict, record->neg_born, record->neg_evict, B, C, Sp, Sn, update ? 1 : 0);
  if (L[3].grid_x) {
    const float pbl2 = params->pos_beta * TILE_LOG2E, nbl2 = params->neg_beta * TILE_LOG2E;
    const TdaSegment g0 = {state->pos_keys, record->pos_born, record->pos_evict, nullptr, nullptr, C * Sp, Sp > 0 ? Sp : 1,
                           params->pos_alpha, pbl2};
    const TdaSegment g1 = {feats, record->pos_born + (size_t)C * Sp, record->pos_evict + (size_t)C * Sp, record->pred, nullptr,
                           Sp > 0 ? B : 0, 1, params->pos_alpha, pbl2};
    const TdaSegment g2 = {state->neg_keys, record->neg_born, record->neg_evict, nullptr, state->neg_mask, C * Sn, 1,
                           -params->neg_alpha, nbl2};
    const TdaSegment g3 = {feats, record->neg_born + (size_t)C * Sn, record->neg_evict + (size_t)C * Sn, nullptr, record->mask,
                           Sn > 0 ? B : 0, 1, -params->neg_alpha, nbl2};
    hipLaunchKernelGGL(tda_logits_kernel, dim3(L[3].grid_x, L[3].grid_y), dim3(L[3].block), 0, st, feats, g0, g1, g2, g3, out, B,
                       C, d, ldout);
  }
  if (L[4].grid_x)
    hipLaunchKernelGGL(tda_write_kernel, dim3(L[4].grid_x), dim3(L[4].block), 0, st, feats, record->pred, record->entropy,
                       (const long long*)record->seq, record->mask, record->pos_slot, record->neg_slot, record->pos_evict,
                       record->neg_evict, state->pos_keys, state->pos_ent, (long long*)state->pos_seq, state->neg_keys,
                       state->neg_ent, (long long*)state->neg_seq, state->neg_mask, (long long*)state->counter, B, C, d, Sp, Sn);
  return launch_status();
}
