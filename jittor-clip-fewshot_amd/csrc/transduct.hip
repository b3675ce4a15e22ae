// Transductive zero-/few-shot inference (clipfs.h "TRANSDUCT"; TransCLIP, Zanella, Gerin and Ben Ayed, NeurIPS 2024), fp32
// in every engine precision mode: the whole unlabelled test set at once, a k-nearest-neighbour affinity among its features
// and a block-wise update of the assignments z, the class means mu and one shared diagonal variance.
//
//   logits   one workgroup per (32 classes, 32 rows): out = alpha A B^T (+ lam add) (+ bias) on v_mfma_f32_32x32x2_f32
//            (tile_dots_staged of logits_tile.h: both operands pass through LDS in chunks of 128 features, wave w taking
//            features [32 w, 32 w + 32) of every chunk, the waves' partials added in wave order).  Used for s F T^T and for
//            u = lam logy + F mu'^T + b.
//   logsm    one wave per row: logy = t - max - log(sum exp(t - max)) in place, the zero-shot label (ties low), z0 = exp(logy).
//   knn      one workgroup per (32 query rows, column chunk) walks the chunk's key tiles of 32 ascending.  The 32 x 32 dots
//            are formed as in `logits` (the next chunk or tile in flight while this one is multiplied); each of the 1024
//            elements that beats its row's current k-th entry (value descending, index ascending: a total order) is queued in
//            LDS, and the row's owner thread inserts the queue into its sorted list in registers.  The result is the top k of a total order, so neither the queue order nor the chunking can
//            change a bit of it.  The similarities never reach memory.
//   merge    (only with more than one chunk) one thread per row inserts the chunks' lists in chunk order.
//   shots    one workgroup per class: gamma M_c and gamma sum_{y_j = c} s_j, shots in ascending j.
//   q        Q_d = sum_i f_id^2 + gamma sum_j s_jd^2, in double, 16 row groups combined in group order.
//   init     one workgroup per 32 classes: 8 row groups each keep a top-m list per class in registers (a row of logy is
//            read 128 bytes at a time), merged in group order; then mu of the 32 classes, var = 1 / d and mu' = mu / var.
//   bias     one wave per class: b_c = -1/2 sum_d mu_cd mu'_cd.
//   z_step   one wave per row: t_c = u_ic + sum_r w_ir z_old[nbr_ir, c] (r ascending), row softmax in registers into the
//            other z buffer; the last sweep also writes argmax z (ties low).
//   stats    G partial = z^T F on the matrix cores: one wave per (32 classes, 32 features), a workgroup's four waves
//            sharing the classes; the rows are cut into `splits` contiguous ranges (grid.z), each walked in ascending pairs.
//            The workgroups of feature chunk 0 also sum z per class.  Partials go to the workspace.
//   muvar    one workgroup per 32 features: combines the partials in split order (then the shots' constants), moves mu where
//            n_c > n_min, accumulates the variance's terms in double over 8 class groups combined in group order, writes
//            n, G, mu, var and mu'.
//
// No float atomics (the kNN queue's counter is an integer in LDS); every output element is written by one thread; every sum
// runs in an order fixed by the shapes.  Nothing returns to the host.
#include "logits_tile.h"

#include <limits.h>
#include <math.h>

namespace clipfs {
namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_K = 8, TR_MAX_M = 16, TR_MAX_CHUNKS = 64, TR_MAX_SPLITS = 8;
constexpr int TR_INIT_GROUPS = 8;   // row groups of an init workgroup
constexpr int TR_Q_THREADS = 1024;  // 64 features x 16 row groups
constexpr int TR_MV_GROUPS = 8;     // class groups of a muvar workgroup

// (a, ja) comes before (b, jb): larger value, ties to the lower index.  A NaN never comes before anything.
__device__ __forceinline__ bool tr_beats(float a, int ja, float b, int jb) { return a > b || (a == b && ja < jb); }

// A sorted list in registers (every index is a compile-time constant after unrolling); empty slots are (-inf, INT_MAX).
template <int CAP>
struct TrList {
  float v[CAP];
  int j[CAP];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int r = 0; r < CAP; ++r) {
      v[r] = -INFINITY;
      j[r] = INT_MAX;
    }
  }
  __device__ __forceinline__ void insert(float a, int ja) {
#pragma unroll
    for (int r = 0; r < CAP; ++r) {
      const bool b = tr_beats(a, ja, v[r], j[r]);
      const float tv = b ? v[r] : a;
      const int tj = b ? j[r] : ja;
      v[r] = b ? a : v[r];
      j[r] = b ? ja : j[r];
      a = tv;
      ja = tj;
    }
  }
  __device__ __forceinline__ void rank(int k, float& kv, int& kj) const {  // entry k - 1
    kv = v[0];
    kj = j[0];
#pragma unroll
    for (int r = 1; r < CAP; ++r)
      if (r == k - 1) {
        kv = v[r];
        kj = j[r];
      }
  }
};

__device__ __forceinline__ int tr_wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// ------------------------------------------------------------------------------------------------- logits / u
__global__ __launch_bounds__(TR_THREADS) void tr_logits_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                               const float* __restrict__ add, const float* __restrict__ bias,
                                                               float* __restrict__ out, int N, int C, int d, float alpha,
                                                               float lam) {
  __shared__ __attribute__((aligned(16))) float sA[32 * TILE_KST];
  __shared__ __attribute__((aligned(16))) float sB[32 * TILE_KST];
  __shared__ float Ps[4][32 * TILE_PS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int c0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  TileStage st;
  st.load(A, b0, N, Bm, c0, C, d, 0, tid);
  const f32x16 acc = tile_dots_staged(st, A, b0, N, Bm, c0, C, d, b0, c0, false, sA, sB, tid);
#pragma unroll
  for (int r = 0; r < 16; ++r) Ps[w][tile_row(r, h) * TILE_PS + li] = acc[r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + TR_THREADS * i, row = e >> 5, col = e & 31;
    if (b0 + row < N && c0 + col < C) {
      const size_t at = (size_t)(b0 + row) * C + c0 + col;
      float v = alpha * tile_sum4(Ps, row * TILE_PS + col);
      if (add) v = lam * add[at] + v;
      if (bias) v = v + bias[c0 + col];
      out[at] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------- log-softmax rows
__global__ __launch_bounds__(TR_THREADS) void tr_logsm_kernel(float* __restrict__ logy, float* __restrict__ z0,
                                                              int32_t* __restrict__ zs, int N, int C) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (TR_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= N) return;  // wave-uniform; no barrier in this kernel
  float* row = logy + (size_t)i * C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
  m = wave_max(m);
  int best = C;
  for (int c = lane; c < C; c += 64)
    if (row[c] == m && c < best) best = c;
  best = tr_wave_min_int(best);
  if (best >= C) best = 0;  // a row that is not numbers: class 0
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(row[c] - m);
  s = wave_sum(s);
  const float ls = logf(s);
  for (int c = lane; c < C; c += 64) {
    const float l = (row[c] - m) - ls;
    row[c] = l;
    z0[(size_t)i * C + c] = expf(l);
  }
  if (lane == 0) zs[i] = best;
}

// ------------------------------------------------------------------------------------------------- kNN
// Lists go to out_v / out_j [gridDim.y, N, k]: the final arrays when there is one chunk, the merge's input otherwise.
__global__ __launch_bounds__(TR_THREADS) void tr_knn_kernel(const float* __restrict__ F, float* __restrict__ out_v,
                                                            int32_t* __restrict__ out_j, int N, int d, int k,
                                                            int tiles_per_chunk, int final_out) {
  __shared__ __attribute__((aligned(16))) float sX[32 * TILE_KST];
  __shared__ __attribute__((aligned(16))) float sY[32 * TILE_KST];
  __shared__ float Ps[4][32 * TILE_PS];
  __shared__ float q_v[32][32];
  __shared__ int q_j[32][32];
  __shared__ int q_n[32], thr_j[32];
  __shared__ float thr_v[32];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * 32, ntiles = (N + 31) / 32;
  const int t0 = min(ntiles, (int)blockIdx.y * tiles_per_chunk), t1 = min(ntiles, t0 + tiles_per_chunk);
  TrList<TR_MAX_K> L;
  L.init();
  if (tid < 32) {
    q_n[tid] = 0;
    thr_v[tid] = -INFINITY;
    thr_j[tid] = INT_MAX;
  }
  TileStage st;
  if (t0 < t1) st.load(F, x0, N, F, t0 * 32, N, d, 0, tid);
  for (int t = t0; t < t1; ++t) {
    const int y0 = t * 32;
    const f32x16 acc = tile_dots_staged(st, F, x0, N, F, y0, N, d, x0, y0 + 32, t + 1 < t1, sX, sY, tid);
#pragma unroll
    for (int r = 0; r < 16; ++r) Ps[w][tile_row(r, h) * TILE_PS + li] = acc[r];
    __syncthreads();  // the partials are there; the owners' update of the last tile (and the initial state) is visible
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + TR_THREADS * i, own = e & 31, oth = e >> 5;
      const float a = tile_sum4(Ps, own * TILE_PS + oth);
      const int xi = x0 + own, yj = y0 + oth;
      if (xi < N && yj < N && yj != xi && tr_beats(a, yj, thr_v[own], thr_j[own])) {
        const int s = atomicAdd(&q_n[own], 1);  // an LDS integer: at most 32 per row and tile
        q_v[own][s] = a;
        q_j[own][s] = yj;
      }
    }
    __syncthreads();
    if (tid < 32) {
      const int n = q_n[tid];
      for (int q = 0; q < n; ++q) L.insert(q_v[tid][q], q_j[tid][q]);
      if (n) {
        float kv;
        int kj;
        L.rank(k, kv, kj);
        thr_v[tid] = kv;
        thr_j[tid] = kj;
        q_n[tid] = 0;
      }
    }
  }
  if (tid < 32 && x0 + tid < N) {
    const size_t at = ((size_t)blockIdx.y * N + x0 + tid) * k;
#pragma unroll
    for (int r = 0; r < TR_MAX_K; ++r)
      if (r < k) {
        const bool empty = L.j[r] >= N;  // possible in a chunk's list; in a final list only for rows that are not numbers
        out_v[at + r] = (final_out && empty) ? 0.f : L.v[r];
        out_j[at + r] = (final_out && empty) ? 0 : L.j[r];
      }
  }
}

__global__ __launch_bounds__(TR_THREADS) void tr_knn_merge_kernel(const float* __restrict__ part_v,
                                                                  const int32_t* __restrict__ part_j, float* __restrict__ w,
                                                                  int32_t* __restrict__ nbr, int N, int k, int chunks) {
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N) return;
  TrList<TR_MAX_K> L;
  L.init();
  for (int c = 0; c < chunks; ++c)
    for (int r = 0; r < k; ++r) {
      const size_t at = ((size_t)c * N + i) * k + r;
      const int j = part_j[at];
      if (j >= 0 && j < N) L.insert(part_v[at], j);
    }
#pragma unroll
  for (int r = 0; r < TR_MAX_K; ++r)
    if (r < k) {
      const bool empty = L.j[r] >= N;
      w[(size_t)i * k + r] = empty ? 0.f : L.v[r];
      nbr[(size_t)i * k + r] = empty ? 0 : L.j[r];
    }
}

// ------------------------------------------------------------------------------------------------- shots' constants
__global__ __launch_bounds__(TR_THREADS) void tr_shots_kernel(const float* __restrict__ S, const int32_t* __restrict__ y,
                                                              float* __restrict__ shot_n, float* __restrict__ shot_G, int M,
                                                              int d, float gamma) {
  __shared__ int cnt[TR_THREADS];
  const int tid = threadIdx.x, c = blockIdx.x;
  int n = 0;
  for (int j = tid; j < M; j += TR_THREADS) n += y[j] == c ? 1 : 0;
  cnt[tid] = n;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int t = 0; t < TR_THREADS; ++t) tot += cnt[t];
    shot_n[c] = gamma * (float)tot;
  }
  for (int dd = tid; dd < d; dd += TR_THREADS) {
    float acc = 0.f;
    for (int j = 0; j < M; ++j)
      if (y[j] == c) acc += S[(size_t)j * d + dd];
    shot_G[(size_t)c * d + dd] = gamma * acc;
  }
}

__global__ __launch_bounds__(TR_Q_THREADS) void tr_q_kernel(const float* __restrict__ F, const float* __restrict__ S,
                                                            float* __restrict__ Q, int N, int M, int d, float gamma) {
  __shared__ double part[2][16][64];
  const int tid = threadIdx.x, fl = tid & 63, g = tid >> 6, dd = blockIdx.x * 64 + fl;
  double qf = 0.0, qs = 0.0;
  if (dd < d) {
    for (int i = g; i < N; i += 16) {
      const double f = (double)F[(size_t)i * d + dd];
      qf += f * f;
    }
    for (int j = g; j < M; j += 16) {
      const double s = (double)S[(size_t)j * d + dd];
      qs += s * s;
    }
  }
  part[0][g][fl] = qf;
  part[1][g][fl] = qs;
  __syncthreads();
  if (g == 0 && dd < d) {
    double a = 0.0, b = 0.0;
    for (int t = 0; t < 16; ++t) {
      a += part[0][t][fl];
      b += part[1][t][fl];
    }
    Q[dd] = (float)(a + (double)gamma * b);
  }
}

// ------------------------------------------------------------------------------------------------- init
__global__ __launch_bounds__(TR_THREADS) void tr_init_kernel(const float* __restrict__ F, const float* __restrict__ logy,
                                                             const float* __restrict__ shot_n, const float* __restrict__ shot_G,
                                                             int32_t* __restrict__ sel, float* __restrict__ mu,
                                                             float* __restrict__ mup, float* __restrict__ var, int N, int C, int d,
                                                             int m) {
  __shared__ float l_v[TR_INIT_GROUPS][32][TR_MAX_M];
  __shared__ int l_j[TR_INIT_GROUPS][32][TR_MAX_M];
  __shared__ int s_sel[32][TR_MAX_M];
  const int tid = threadIdx.x, cl = tid & 31, g = tid >> 5, c0 = blockIdx.x * 32;
  const int c = min(c0 + cl, C - 1);
  TrList<TR_MAX_M> L;
  L.init();
  float kv = -INFINITY;
  int kj = INT_MAX;
  for (int i = g; i < N; i += TR_INIT_GROUPS) {
    const float a = logy[(size_t)i * C + c];
    if (tr_beats(a, i, kv, kj)) {
      L.insert(a, i);
      L.rank(m, kv, kj);
    }
  }
#pragma unroll
  for (int r = 0; r < TR_MAX_M; ++r) {
    l_v[g][cl][r] = L.v[r];
    l_j[g][cl][r] = L.j[r];
  }
  __syncthreads();
  if (g == 0) {
    for (int g2 = 1; g2 < TR_INIT_GROUPS; ++g2)
      for (int r = 0; r < TR_MAX_M; ++r) L.insert(l_v[g2][cl][r], l_j[g2][cl][r]);
#pragma unroll
    for (int r = 0; r < TR_MAX_M; ++r) {
      const int j = min(max(L.j[r], 0), N - 1);  // out of range only for a column that is not numbers
      s_sel[cl][r] = j;
      if (r < m && c0 + cl < C) sel[(size_t)(c0 + cl) * m + r] = j;
    }
  }
  __syncthreads();
  const float v0 = 1.f / (float)d;
  const int nc = min(32, C - c0);
  for (int e = tid; e < nc * d; e += TR_THREADS) {
    const int ci = e / d, dd = e - ci * d, cc = c0 + ci;
    float acc = 0.f;
    for (int r = 0; r < m; ++r) acc += F[(size_t)s_sel[ci][r] * d + dd];
    acc += shot_G[(size_t)cc * d + dd];
    const float mm = acc / ((float)m + shot_n[cc]);
    mu[(size_t)cc * d + dd] = mm;
    mup[(size_t)cc * d + dd] = mm / v0;
  }
  if (blockIdx.x == 0)
    for (int dd = tid; dd < d; dd += TR_THREADS) var[dd] = v0;
}

// ------------------------------------------------------------------------------------------------- bias
__global__ __launch_bounds__(TR_THREADS) void tr_bias_kernel(const float* __restrict__ mu, const float* __restrict__ mup,
                                                             float* __restrict__ bias, int C, int d) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * (TR_THREADS / 64) + (threadIdx.x >> 6);
  if (c >= C) return;  // wave-uniform
  float acc = 0.f;
  for (int dd = lane; dd < d; dd += 64) acc += mu[(size_t)c * d + dd] * mup[(size_t)c * d + dd];
  acc = wave_sum(acc);
  if (lane == 0) bias[c] = -0.5f * acc;
}

// ------------------------------------------------------------------------------------------------- z sweep
// NV: classes per lane, C <= 64 NV.  A neighbour index outside [0, N) is clamped (the kNN launch never writes one).
template <int NV>
__global__ __launch_bounds__(TR_THREADS) void tr_z_step_kernel(const float* __restrict__ u, const int32_t* __restrict__ nbr,
                                                               const float* __restrict__ w, const float* __restrict__ z_in,
                                                               float* __restrict__ z_out, int32_t* __restrict__ labels, int N,
                                                               int C, int k) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (TR_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= N) return;  // wave-uniform; no barrier in this kernel
  const float* zr[TR_MAX_K];
  float wr[TR_MAX_K];
#pragma unroll
  for (int r = 0; r < TR_MAX_K; ++r) {
    const int rr = min(r, k - 1);
    const int j = min(max(nbr[(size_t)i * k + rr], 0), N - 1);
    zr[r] = z_in + (size_t)j * C;
    wr[r] = r < k ? w[(size_t)i * k + rr] : 0.f;
  }
  const float* ur = u + (size_t)i * C;
  float t[NV];
  float m = -INFINITY;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = lane + 64 * v;
    t[v] = -INFINITY;
    if (c < C) {
      float a = ur[c];
#pragma unroll
      for (int r = 0; r < TR_MAX_K; ++r)
        if (r < k) a += wr[r] * zr[r][c];
      t[v] = a;
      m = fmaxf(m, a);
    }
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = lane + 64 * v;
    if (c < C) {
      t[v] = expf(t[v] - m);
      s += t[v];
    }
  }
  s = wave_sum(s);
  float bv = -INFINITY;
  int bc = C;
  float* zo = z_out + (size_t)i * C;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = lane + 64 * v;
    if (c < C) {
      const float zz = t[v] / s;
      zo[c] = zz;
      if (zz > bv) {  // ascending c: the first of equals stays
        bv = zz;
        bc = c;
      }
    }
  }
  if (labels) {
    const float bm = wave_max(bv);
    int best = tr_wave_min_int(bv == bm ? bc : C);
    if (best >= C) best = 0;
    if (lane == 0) labels[i] = best;
  }
}

// ------------------------------------------------------------------------------------------------- class statistics
// grid (32-class tiles, 128-feature chunks, splits).  Lane (li, h) of wave w feeds z[i + h][c0 + li] and
// F[i + h][f0 + 32 w + li] for the row pairs i = r0, r0 + 2, ... of its split; rows >= N contribute zeros.
__global__ __launch_bounds__(TR_THREADS) void tr_stats_kernel(const float* __restrict__ z, const float* __restrict__ F,
                                                              float* __restrict__ part_G, float* __restrict__ part_n, int N, int C,
                                                              int d, int rows_per_split) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int c0 = blockIdx.x * 32, f0 = blockIdx.y * 128 + 32 * w, p = blockIdx.z;
  const int r0 = p * rows_per_split, r1 = min(N, r0 + rows_per_split);
  const int cz = min(c0 + li, C - 1), ff = min(f0 + li, d - 1);
  const bool live = f0 < d;  // wave-uniform
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float nacc = 0.f;
  if (live) {
    for (int i = r0; i < r1; i += 16) {
      float a[8], b[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int row = i + 2 * s + h;
        const bool in = row < r1;
        const size_t rr = (size_t)(in ? row : r1 - 1);
        const float za = z[rr * C + cz], fb = F[rr * d + ff];
        a[s] = in ? za : 0.f;
        b[s] = in ? fb : 0.f;
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        acc = tile_mfma(a[s], b[s], acc);
        nacc += a[s];
      }
    }
    if (f0 + li < d) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cc = c0 + tile_row(r, h);
        if (cc < C) part_G[((size_t)p * C + cc) * d + f0 + li] = acc[r];
      }
    }
  }
  if (blockIdx.y == 0 && w == 0) {
    const float other = __shfl_xor(nacc, 32, 64);
    if (h == 0 && c0 + li < C) part_n[(size_t)p * C + c0 + li] = nacc + other;  // even rows' sum + odd rows' sum
  }
}

__global__ __launch_bounds__(TR_THREADS) void tr_muvar_kernel(const float* __restrict__ part_G, const float* __restrict__ part_n,
                                                              const float* __restrict__ shot_n, const float* __restrict__ shot_G,
                                                              const float* __restrict__ Q, float* __restrict__ n_out,
                                                              float* __restrict__ G, float* __restrict__ mu, float* __restrict__ var,
                                                              float* __restrict__ mup, int C, int d, int splits, float n_min,
                                                              float var_floor, double denom) {
  __shared__ double ts[TR_MV_GROUPS][32];
  const int tid = threadIdx.x, fl = tid & 31, g = tid >> 5, dd = blockIdx.x * 32 + fl;
  const int per = (C + TR_MV_GROUPS - 1) / TR_MV_GROUPS, c_lo = min(C, g * per), c_hi = min(C, c_lo + per);
  const bool own = dd < d;
  double t = 0.0;
  if (own) {
    for (int c = c_lo; c < c_hi; ++c) {
      float nn = 0.f, gg = 0.f;
      for (int p = 0; p < splits; ++p) {
        nn += part_n[(size_t)p * C + c];
        gg += part_G[((size_t)p * C + c) * d + dd];
      }
      nn += shot_n[c];
      gg += shot_G[(size_t)c * d + dd];
      const size_t at = (size_t)c * d + dd;
      float mm = mu[at];
      if (nn > n_min) mm = gg / nn;
      mu[at] = mm;
      G[at] = gg;
      if (dd == 0) n_out[c] = nn;
      t += (double)nn * (double)mm * (double)mm - 2.0 * (double)mm * (double)gg;
    }
  }
  ts[g][fl] = t;
  __syncthreads();
  if (own) {
    double tot = (double)Q[dd];
    for (int g2 = 0; g2 < TR_MV_GROUPS; ++g2) tot += ts[g2][fl];
    const float v = fmaxf(var_floor, (float)(tot / denom));
    if (g == 0) var[dd] = v;
    for (int c = c_lo; c < c_hi; ++c) mup[(size_t)c * d + dd] = mu[(size_t)c * d + dd] / v;  // mu: this thread's own stores
  }
}

// ------------------------------------------------------------------------------------------------- host
typedef struct clipfs_transduct_params TrParams;
typedef struct clipfs_transduct_buffers TrBufs;
typedef struct clipfs_transduct_plan TrPlan;

bool tr_ok_scalar(float v) { return isfinite(v) && v >= 0.f; }

int tr_check_params(const TrParams* p, const char* who) {
  CLIPFS_REQUIRE(p != nullptr, "%s: NULL params", who);
  CLIPFS_REQUIRE(p->struct_size == sizeof(TrParams), "%s: params.struct_size = %u, this library expects %u", who, p->struct_size,
                 (unsigned)sizeof(TrParams));
  CLIPFS_REQUIRE(p->d >= 4 && p->d <= 4096 && p->d % 4 == 0, "%s: d = %d must be a multiple of 4 in [4, 4096]", who, p->d);
  CLIPFS_REQUIRE(p->C >= 1 && p->C <= 4096, "%s: C = %d outside [1, 4096]", who, p->C);
  CLIPFS_REQUIRE(p->k >= 1 && p->k <= TR_MAX_K, "%s: k = %d outside [1, %d]", who, p->k, TR_MAX_K);
  CLIPFS_REQUIRE(p->init_top >= 1 && p->init_top <= TR_MAX_M, "%s: init_top = %d outside [1, %d]", who, p->init_top, TR_MAX_M);
  const int n_lo = p->k + 1 > p->init_top ? p->k + 1 : p->init_top;
  CLIPFS_REQUIRE(p->N >= n_lo && p->N <= 131072, "%s: N = %d outside [max(k + 1, init_top) = %d, 131072]", who, p->N, n_lo);
  CLIPFS_REQUIRE(p->M >= 0 && p->M <= 65536, "%s: M = %d outside [0, 65536]", who, p->M);
  CLIPFS_REQUIRE(p->outer >= 1, "%s: outer = %d must be >= 1", who, p->outer);
  CLIPFS_REQUIRE(p->inner >= 1, "%s: inner = %d must be >= 1", who, p->inner);
  CLIPFS_REQUIRE((long long)p->outer * p->inner <= 1000000, "%s: outer * inner = %lld above 1000000", who,
                 (long long)p->outer * p->inner);
  CLIPFS_REQUIRE(p->knn_chunks >= 0 && p->knn_chunks <= TR_MAX_CHUNKS, "%s: knn_chunks = %d outside [0, %d] (0: the plan decides)",
                 who, p->knn_chunks, TR_MAX_CHUNKS);
  CLIPFS_REQUIRE(tr_ok_scalar(p->logit_scale), "%s: logit_scale = %g must be finite and >= 0", who, (double)p->logit_scale);
  CLIPFS_REQUIRE(tr_ok_scalar(p->lam), "%s: lam = %g must be finite and >= 0", who, (double)p->lam);
  CLIPFS_REQUIRE(tr_ok_scalar(p->shot_weight), "%s: shot_weight = %g must be finite and >= 0", who, (double)p->shot_weight);
  CLIPFS_REQUIRE(tr_ok_scalar(p->n_min), "%s: n_min = %g must be finite and >= 0", who, (double)p->n_min);
  CLIPFS_REQUIRE(tr_ok_scalar(p->var_floor) && p->var_floor > 0.f, "%s: var_floor = %g must be finite and > 0", who,
                 (double)p->var_floor);
  return CLIPFS_OK;
}

int tr_check_bufs(const TrBufs* b, const char* who) {
  CLIPFS_REQUIRE(b != nullptr, "%s: NULL buffers", who);
  CLIPFS_REQUIRE(b->struct_size == sizeof(TrBufs), "%s: buffers.struct_size = %u, this library expects %u", who, b->struct_size,
                 (unsigned)sizeof(TrBufs));
  return CLIPFS_OK;
}

// One member of the buffers a stage uses: its name, address, size and whether the stage writes it.
struct TrSpan {
  const char* name;
  const void* p;
  size_t bytes;
  bool written, align16;
};

int tr_check_spans(const TrSpan* s, int n, const char* who) {
  for (int i = 0; i < n; ++i) {
    if (s[i].bytes == 0) continue;
    CLIPFS_REQUIRE(s[i].p != nullptr, "%s: %s is NULL", who, s[i].name);
    const uintptr_t a = reinterpret_cast<uintptr_t>(s[i].p);
    CLIPFS_REQUIRE((a & (s[i].align16 ? 15u : 3u)) == 0, "%s: %s is not %d-byte aligned", who, s[i].name, s[i].align16 ? 16 : 4);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      if (i == j || !s[i].written || !s[i].bytes || !s[j].bytes) continue;
      const uintptr_t a = reinterpret_cast<uintptr_t>(s[i].p), b = reinterpret_cast<uintptr_t>(s[j].p);
      CLIPFS_REQUIRE(!(a < b + s[j].bytes && b < a + s[i].bytes), "%s: %s aliases %s", who, s[i].name, s[j].name);
    }
  return CLIPFS_OK;
}

int tr_check_labels(const TrParams* p, const TrBufs* b, const char* who) {
  if (p->M > 0 && b->shot_labels_host)
    for (int j = 0; j < p->M; ++j)
      CLIPFS_REQUIRE(b->shot_labels_host[j] >= 0 && b->shot_labels_host[j] < p->C,
                     "%s: shot_labels[%d] = %d outside [0, C = %d)", who, j, b->shot_labels_host[j], p->C);
  return CLIPFS_OK;
}

#define TR_LAUNCH(kernel, L, st, ...) \
  hipLaunchKernelGGL(kernel, dim3((L).grid_x, (L).grid_y, (L).grid_z), dim3((L).block), 0, st, __VA_ARGS__)

// ---- the stages, unchecked: the entry points and the fit check first and then call these
void tr_run_logy(const TrParams* p, const TrPlan& pl, const TrBufs* b, float* z0, hipStream_t st) {
  TR_LAUNCH(tr_logits_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_LOGITS], st, b->feats, b->text, (const float*)nullptr,
            (const float*)nullptr, b->logy, p->N, p->C, p->d, p->logit_scale, 0.f);
  TR_LAUNCH(tr_logsm_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_LOGSM], st, b->logy, z0, b->zs_labels, p->N, p->C);
}

void tr_run_knn(const TrParams* p, const TrPlan& pl, const TrBufs* b, hipStream_t st) {
  const int ntiles = (p->N + 31) / 32, per = (ntiles + pl.knn_chunks - 1) / pl.knn_chunks;
  if (pl.knn_chunks == 1) {
    TR_LAUNCH(tr_knn_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_KNN], st, b->feats, b->w, b->nbr, p->N, p->d, p->k, per, 1);
  } else {
    float* pv = (float*)b->knn_work;
    int32_t* pj = (int32_t*)(pv + (size_t)pl.knn_chunks * p->N * p->k);
    TR_LAUNCH(tr_knn_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_KNN], st, b->feats, pv, pj, p->N, p->d, p->k, per, 0);
    TR_LAUNCH(tr_knn_merge_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_KNN_MERGE], st, (const float*)pv, (const int32_t*)pj, b->w,
              b->nbr, p->N, p->k, pl.knn_chunks);
  }
}

void tr_run_init(const TrParams* p, const TrPlan& pl, const TrBufs* b, hipStream_t st) {
  TR_LAUNCH(tr_shots_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_SHOTS], st, b->shots, b->shot_labels, b->shot_n, b->shot_G, p->M,
            p->d, p->shot_weight);
  TR_LAUNCH(tr_q_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_Q], st, b->feats, b->shots, b->Q, p->N, p->M, p->d, p->shot_weight);
  TR_LAUNCH(tr_init_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_INIT], st, b->feats, (const float*)b->logy, (const float*)b->shot_n,
            (const float*)b->shot_G, b->sel, b->mu, b->mup, b->var, p->N, p->C, p->d, p->init_top);
}

void tr_run_u(const TrParams* p, const TrPlan& pl, const TrBufs* b, hipStream_t st) {
  TR_LAUNCH(tr_bias_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_BIAS], st, (const float*)b->mu, (const float*)b->mup, b->bias, p->C,
            p->d);
  TR_LAUNCH(tr_logits_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_U], st, b->feats, (const float*)b->mup, (const float*)b->logy,
            (const float*)b->bias, b->u, p->N, p->C, p->d, 1.f, p->lam);
}

void tr_run_z_step(const TrParams* p, const TrPlan& pl, const TrBufs* b, const float* z_in, float* z_out, int32_t* labels,
                   hipStream_t st) {
  const struct clipfs_transduct_launch& L = pl.launch[CLIPFS_TRANSDUCT_LAUNCH_Z_STEP];
  if (pl.class_chunk == 256)
    TR_LAUNCH(tr_z_step_kernel<4>, L, st, (const float*)b->u, (const int32_t*)b->nbr, (const float*)b->w, z_in, z_out, labels, p->N,
              p->C, p->k);
  else if (pl.class_chunk == 1024)
    TR_LAUNCH(tr_z_step_kernel<16>, L, st, (const float*)b->u, (const int32_t*)b->nbr, (const float*)b->w, z_in, z_out, labels,
              p->N, p->C, p->k);
  else
    TR_LAUNCH(tr_z_step_kernel<64>, L, st, (const float*)b->u, (const int32_t*)b->nbr, (const float*)b->w, z_in, z_out, labels,
              p->N, p->C, p->k);
}

void tr_run_stats(const TrParams* p, const TrPlan& pl, const TrBufs* b, const float* z_in, hipStream_t st) {
  float* pg = b->stat_work;
  float* pn = pg + (size_t)pl.stat_splits * p->C * p->d;
  TR_LAUNCH(tr_stats_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_STATS], st, z_in, b->feats, pg, pn, p->N, p->C, p->d,
            pl.stat_rows);
  TR_LAUNCH(tr_muvar_kernel, pl.launch[CLIPFS_TRANSDUCT_LAUNCH_MUVAR], st, (const float*)pg, (const float*)pn,
            (const float*)b->shot_n, (const float*)b->shot_G, (const float*)b->Q, b->n, b->G, b->mu, b->var, b->mup, p->C, p->d,
            pl.stat_splits, p->n_min, p->var_floor, (double)p->N + (double)p->shot_weight * (double)p->M);
}

// the spans of the members named by `mask` bits, in the order of TrField
enum TrField {
  TF_FEATS, TF_TEXT, TF_SHOTS, TF_YLAB, TF_Z, TF_LABELS, TF_ZS, TF_MU, TF_VAR, TF_NBR, TF_W, TF_LOGY, TF_U, TF_Z2, TF_MUP,
  TF_BIAS, TF_N, TF_G, TF_Q, TF_SHOT_N, TF_SHOT_G, TF_SEL, TF_STAT_WORK, TF_KNN_WORK, TF_COUNT
};

int tr_spans(const TrParams* p, const TrPlan& pl, const TrBufs* b, unsigned used, unsigned written, const char* who) {
  const size_t N = p->N, C = p->C, d = p->d, M = p->M, k = p->k;
  const TrSpan all[TF_COUNT] = {
      {"feats", b->feats, N * d * 4, false, true},
      {"text", b->text, C * d * 4, false, true},
      {"shots", b->shots, M * d * 4, false, true},
      {"shot_labels", b->shot_labels, M * 4, false, false},
      {"z", b->z, N * C * 4, false, true},
      {"labels", b->labels, N * 4, false, false},
      {"zs_labels", b->zs_labels, N * 4, false, false},
      {"mu", b->mu, C * d * 4, false, true},
      {"var", b->var, d * 4, false, false},
      {"nbr", b->nbr, N * k * 4, false, false},
      {"w", b->w, N * k * 4, false, false},
      {"logy", b->logy, N * C * 4, false, true},
      {"u", b->u, N * C * 4, false, true},
      {"z2", b->z2, N * C * 4, false, true},
      {"mup", b->mup, C * d * 4, false, true},
      {"bias", b->bias, C * 4, false, false},
      {"n", b->n, C * 4, false, false},
      {"G", b->G, C * d * 4, false, true},
      {"Q", b->Q, d * 4, false, false},
      {"shot_n", b->shot_n, C * 4, false, false},
      {"shot_G", b->shot_G, C * d * 4, false, true},
      {"sel", b->sel, C * (size_t)p->init_top * 4, false, false},
      {"stat_work", b->stat_work, pl.stat_work_floats * 4, false, true},
      {"knn_work", b->knn_work, pl.knn_work_bytes, false, true},
  };
  TrSpan s[TF_COUNT];
  int n = 0;
  for (int f = 0; f < TF_COUNT; ++f)
    if (used & (1u << f)) {
      s[n] = all[f];
      s[n].written = (written & (1u << f)) != 0;
      ++n;
    }
  return tr_check_spans(s, n, who);
}

#define TF(x) (1u << TF_##x)

// `z_in` / `z_out` of the stages that take them: checked like members
int tr_check_extra(const void* p, size_t bytes, const char* name, const char* who) {
  CLIPFS_REQUIRE(p != nullptr, "%s: %s is NULL", who, name);
  CLIPFS_REQUIRE(aligned16(p), "%s: %s is not 16-byte aligned", who, name);
  (void)bytes;
  return CLIPFS_OK;
}

bool tr_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_transduct_plan(const struct clipfs_transduct_params* params, struct clipfs_transduct_plan* plan) {
  CLIPFS_REQUIRE(plan != nullptr, "clipfs_transduct_plan: NULL plan");
  CLIPFS_CHECK(tr_check_params(params, "clipfs_transduct_plan"));
  const int N = params->N, C = params->C, d = params->d, k = params->k;
  TrPlan p = {};
  const unsigned rt = (unsigned)((N + 31) / 32), ct = (unsigned)((C + 31) / 32);
  const unsigned tile_lds = (unsigned)((2 * 32 * TILE_KST + 4 * 32 * TILE_PS) * sizeof(float));  // staged operands + partials
  // column chunks of the kNN walk: one where the row tiles alone give every compute unit a workgroup; else enough for
  // about two workgroups per unit, never more than the key tiles
  int chunks = params->knn_chunks;
  if (chunks == 0) {
    chunks = rt >= 256 ? 1 : (int)((512 + rt - 1) / rt);
    if (chunks > (int)rt) chunks = (int)rt;
    if (chunks > TR_MAX_CHUNKS) chunks = TR_MAX_CHUNKS;
  }
  p.knn_chunks = chunks;
  p.class_chunk = C <= 256 ? 256 : C <= 1024 ? 1024 : 4096;
  const unsigned fchunks = (unsigned)((d + 127) / 128);
  int splits = (int)((512 + ct * fchunks - 1) / (ct * fchunks));
  if (splits > TR_MAX_SPLITS) splits = TR_MAX_SPLITS;
  if (splits > (N + 63) / 64) splits = (N + 63) / 64;
  if (splits < 1) splits = 1;
  p.stat_rows = ((N + splits - 1) / splits + 15) / 16 * 16;
  p.stat_splits = (N + p.stat_rows - 1) / p.stat_rows;
  struct clipfs_transduct_launch* L = p.launch;
  L[CLIPFS_TRANSDUCT_LAUNCH_LOGITS] = {ct, rt, 1, TR_THREADS, tile_lds};
  L[CLIPFS_TRANSDUCT_LAUNCH_LOGSM] = {(unsigned)((N + 3) / 4), 1, 1, TR_THREADS, 0};
  L[CLIPFS_TRANSDUCT_LAUNCH_KNN] = {rt, (unsigned)chunks, 1, TR_THREADS,
                                    (unsigned)(tile_lds + (2 * 32 * 32 + 3 * 32) * sizeof(float))};
  if (chunks > 1) L[CLIPFS_TRANSDUCT_LAUNCH_KNN_MERGE] = {(unsigned)((N + TR_THREADS - 1) / TR_THREADS), 1, 1, TR_THREADS, 0};
  L[CLIPFS_TRANSDUCT_LAUNCH_SHOTS] = {(unsigned)C, 1, 1, TR_THREADS, (unsigned)(TR_THREADS * sizeof(int))};
  L[CLIPFS_TRANSDUCT_LAUNCH_Q] = {(unsigned)((d + 63) / 64), 1, 1, TR_Q_THREADS, (unsigned)(2 * 16 * 64 * sizeof(double))};
  L[CLIPFS_TRANSDUCT_LAUNCH_INIT] = {ct, 1, 1, TR_THREADS,
                                     (unsigned)((2 * TR_INIT_GROUPS * 32 * TR_MAX_M + 32 * TR_MAX_M) * sizeof(float))};
  L[CLIPFS_TRANSDUCT_LAUNCH_BIAS] = {(unsigned)((C + 3) / 4), 1, 1, TR_THREADS, 0};
  L[CLIPFS_TRANSDUCT_LAUNCH_U] = {ct, rt, 1, TR_THREADS, tile_lds};
  L[CLIPFS_TRANSDUCT_LAUNCH_Z_STEP] = {(unsigned)((N + 3) / 4), 1, 1, TR_THREADS, 0};
  L[CLIPFS_TRANSDUCT_LAUNCH_STATS] = {ct, fchunks, (unsigned)p.stat_splits, TR_THREADS, 0};
  L[CLIPFS_TRANSDUCT_LAUNCH_MUVAR] = {(unsigned)((d + 31) / 32), 1, 1, TR_THREADS,
                                      (unsigned)(TR_MV_GROUPS * 32 * sizeof(double))};
  for (int i = 0; i < CLIPFS_TRANSDUCT_LAUNCHES; ++i)
    if (L[i].lds_bytes > p.lds_bytes) p.lds_bytes = L[i].lds_bytes;
  // logits, logsm, knn (+ merge), shots, q, init; per outer iteration bias, u, `inner` sweeps, stats, muvar
  p.launches = 6 + (chunks > 1 ? 1 : 0) + params->outer * (params->inner + 4);
  p.knn_work_bytes = chunks > 1 ? (size_t)chunks * N * k * 8 : 0;
  p.stat_work_floats = (size_t)p.stat_splits * C * ((size_t)d + 1);
  p.nc_floats = (size_t)N * C;
  *plan = p;
  return CLIPFS_OK;
}

extern "C" int clipfs_transduct_logy(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* b,
                                     void* stream) {
  TrPlan pl;
  CLIPFS_CHECK(clipfs_transduct_plan(params, &pl));
  CLIPFS_CHECK(tr_check_bufs(b, "clipfs_transduct_logy"));
  CLIPFS_CHECK(tr_spans(params, pl, b, TF(FEATS) | TF(TEXT) | TF(LOGY) | TF(Z) | TF(ZS), TF(LOGY) | TF(Z) | TF(ZS),
                        "clipfs_transduct_logy"));
  tr_run_logy(params, pl, b, b->z, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_transduct_knn(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* b,
                                    void* stream) {
  TrPlan pl;
  CLIPFS_CHECK(clipfs_transduct_plan(params, &pl));
  CLIPFS_CHECK(tr_check_bufs(b, "clipfs_transduct_knn"));
  CLIPFS_CHECK(tr_spans(params, pl, b, TF(FEATS) | TF(NBR) | TF(W) | TF(KNN_WORK), TF(NBR) | TF(W) | TF(KNN_WORK),
                        "clipfs_transduct_knn"));
  tr_run_knn(params, pl, b, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_transduct_init(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* b,
                                     void* stream) {
  TrPlan pl;
  CLIPFS_CHECK(clipfs_transduct_plan(params, &pl));
  CLIPFS_CHECK(tr_check_bufs(b, "clipfs_transduct_init"));
  const unsigned wr = TF(SHOT_N) | TF(SHOT_G) | TF(Q) | TF(SEL) | TF(MU) | TF(MUP) | TF(VAR);
  CLIPFS_CHECK(tr_spans(params, pl, b, TF(FEATS) | TF(SHOTS) | TF(YLAB) | TF(LOGY) | wr, wr, "clipfs_transduct_init"));
  CLIPFS_CHECK(tr_check_labels(params, b, "clipfs_transduct_init"));
  tr_run_init(params, pl, b, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_transduct_u(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* b,
                                  void* stream) {
  TrPlan pl;
  CLIPFS_CHECK(clipfs_transduct_plan(params, &pl));
  CLIPFS_CHECK(tr_check_bufs(b, "clipfs_transduct_u"));
  CLIPFS_CHECK(tr_spans(params, pl, b, TF(FEATS) | TF(LOGY) | TF(MU) | TF(MUP) | TF(BIAS) | TF(U), TF(BIAS) | TF(U),
                        "clipfs_transduct_u"));
  tr_run_u(params, pl, b, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_transduct_z_step(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* b,
                                       const float* z_in, float* z_out, int32_t* labels, void* stream) {
  TrPlan pl;
  CLIPFS_CHECK(clipfs_transduct_plan(params, &pl));
  CLIPFS_CHECK(tr_check_bufs(b, "clipfs_transduct_z_step"));
  CLIPFS_CHECK(tr_spans(params, pl, b, TF(U) | TF(NBR) | TF(W), 0, "clipfs_transduct_z_step"));
  CLIPFS_CHECK(tr_check_extra(z_in, pl.nc_floats * 4, "z_in", "clipfs_transduct_z_step"));
  CLIPFS_CHECK(tr_check_extra(z_out, pl.nc_floats * 4, "z_out", "clipfs_transduct_z_step"));
  const size_t nc = pl.nc_floats * 4;
  CLIPFS_REQUIRE(!tr_overlap(z_out, nc, z_in, nc) && !tr_overlap(z_out, nc, b->u, nc) &&
                     !tr_overlap(z_out, nc, b->nbr, (size_t)params->N * params->k * 4) &&
                     !tr_overlap(z_out, nc, b->w, (size_t)params->N * params->k * 4),
                 "clipfs_transduct_z_step: z_out aliases z_in, u, nbr or w (the sweep is Jacobi: it needs two z buffers)");
  tr_run_z_step(params, pl, b, z_in, z_out, labels, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_transduct_stats(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* b,
                                      const float* z_in, void* stream) {
  TrPlan pl;
  CLIPFS_CHECK(clipfs_transduct_plan(params, &pl));
  CLIPFS_CHECK(tr_check_bufs(b, "clipfs_transduct_stats"));
  const unsigned wr = TF(N) | TF(G) | TF(MU) | TF(VAR) | TF(MUP) | TF(STAT_WORK);
  CLIPFS_CHECK(tr_spans(params, pl, b, TF(FEATS) | TF(SHOT_N) | TF(SHOT_G) | TF(Q) | wr, wr, "clipfs_transduct_stats"));
  CLIPFS_CHECK(tr_check_extra(z_in, pl.nc_floats * 4, "z_in", "clipfs_transduct_stats"));
  tr_run_stats(params, pl, b, z_in, (hipStream_t)stream);
  return launch_status();
}

extern "C" int clipfs_transduct_fit(const struct clipfs_transduct_params* params, const struct clipfs_transduct_buffers* b,
                                    void* stream) {
  TrPlan pl;
  CLIPFS_CHECK(clipfs_transduct_plan(params, &pl));
  CLIPFS_CHECK(tr_check_bufs(b, "clipfs_transduct_fit"));
  const unsigned in = TF(FEATS) | TF(TEXT) | TF(SHOTS) | TF(YLAB);
  const unsigned all = (1u << TF_COUNT) - 1u;
  CLIPFS_CHECK(tr_spans(params, pl, b, all, all & ~in, "clipfs_transduct_fit"));
  CLIPFS_CHECK(tr_check_labels(params, b, "clipfs_transduct_fit"));
  hipStream_t st = (hipStream_t)stream;
  const int sweeps = params->outer * params->inner;
  // the sweeps alternate between z and z2 and the last one must land in z
  float* cur = (sweeps % 2 == 0) ? b->z : b->z2;
  float* oth = (sweeps % 2 == 0) ? b->z2 : b->z;
  tr_run_logy(params, pl, b, cur, st);
  tr_run_knn(params, pl, b, st);
  tr_run_init(params, pl, b, st);
  int done = 0;
  for (int o = 0; o < params->outer; ++o) {
    tr_run_u(params, pl, b, st);
    for (int i = 0; i < params->inner; ++i) {
      ++done;
      tr_run_z_step(params, pl, b, cur, oth, done == sweeps ? b->labels : nullptr, st);
      float* t = cur;
      cur = oth;
      oth = t;
    }
    tr_run_stats(params, pl, b, cur, st);
  }
  return launch_status();
}
