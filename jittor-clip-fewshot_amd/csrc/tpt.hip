// Test-time prompt tuning objective (clipfs.h "TPT objective"; Shu et al., NeurIPS 2022), fp32 in every engine
// precision mode: the entropy of the prediction averaged over the K most confident views of an image and its gradient
// with respect to the class features, for a batch of independent images.
//
//   z_v = s F_v T^T    p_v = softmax(z_v)    H_v = entropy(p_v)    S = the K views of lowest H (ties to the lower index)
//   pbar = (1/K) sum_{v in S} p_v    loss = -sum_c pbar_c log pbar_c    g_c = -log pbar_c
//   dz_v = (1/K) p_v (g - <p_v, g>)  (v in S)    dT = s sum_{v in S} dz_v^T F_v
//
// Three launches whatever n_img (two without the gradient), the grid's last dimension being the image; no float atomics,
// every float is written by one thread and every sum runs in an order fixed by the shapes, so results are bitwise equal
// run to run and an image's results do not depend on the batch around it.
//
//   logits  one workgroup per (32 classes, 32 views, image) forms its tile on v_mfma_f32_32x32x2_f32 (tile_dots of
//           logits_tile.h: rows read straight from global memory / L2, 128 contiguous bytes per lane and 64-feature
//           step); the four waves split the 64-feature steps and their partials are added in wave order.  Every element
//           of a tile sums the same features in the same order: a row's logits do not depend on where the row sits,
//           which is what makes the tie rule exact.
//   reduce  one 1024-thread workgroup per image, in the manner of mta_kernel: a wave per row for max / sum / entropy,
//           a thread per view for the rank count, a thread per class for pbar, g and the loss, a wave per selected row for
//           dz.  Softmax probabilities are recomputed as exp(z - max) / sum wherever they are needed.
//   grad    the rank-K product dz^T F on the VALU, a thread per (class, 4 features), the K terms added in ascending view
//           index.  K is about 6: twelve flops per output element, the launch is bound by its stores.
#include "logits_tile.h"

#include <math.h>

namespace clipfs {
namespace {

constexpr int TPT_MAX_V = 1024;
constexpr int TPT_MAX_D = 1024;
constexpr int TPT_THREADS = 256;       // logits and gradient workgroups: 4 waves
constexpr int TPT_RED_THREADS = 1024;  // the reduction workgroup: one thread per view
constexpr int TPT_GC = 8;              // classes per gradient workgroup

__device__ __forceinline__ float tpt_block_sum(float v, float* red, int tid) {
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < TPT_RED_THREADS / 64; ++w) t += red[w];
  return t;
}

// ------------------------------------------------------------------------------------------------- logits
// z[img, v, c] = s F[img, v, :] . T[c, :] into the first V * C floats of the image's work record.
__global__ __launch_bounds__(TPT_THREADS) void tpt_logits_kernel(const float* __restrict__ feats,
                                                                 const float* __restrict__ text, size_t text_stride,
                                                                 float* __restrict__ work, size_t work_stride, int V, int d,
                                                                 int C, float s) {
  __shared__ float Ps[4][32 * TILE_PS];  // per wave: [view][class] partial over its 64-feature steps
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, h = lane >> 5;
  const int c0 = blockIdx.x * 32, v0 = blockIdx.y * 32, img = blockIdx.z;
  const float* F = feats + (size_t)img * V * d;
  const float* T = text + (size_t)img * text_stride;
  float* z = work + (size_t)img * work_stride;
  const f32x16 acc = tile_dots(F, v0, V, T, c0, C, d, 64 * w, 256, lane);  // this wave's steps; edge products are never stored
#pragma unroll
  for (int r = 0; r < 16; ++r) Ps[w][tile_row(r, h) * TILE_PS + li] = acc[r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + TPT_THREADS * i, row = e >> 5, col = e & 31;
    const float a = tile_sum4(Ps, row * TILE_PS + col);
    if (v0 + row < V && c0 + col < C) z[(size_t)(v0 + row) * C + c0 + col] = s * a;
  }
}

// ------------------------------------------------------------------------------------------------- reduce
// The image's work record: z [V, C] | dz [V, C] (rows 0 .. K - 1 used: the selected views in ascending index) | g [C].
__global__ __launch_bounds__(TPT_RED_THREADS) void tpt_reduce_kernel(float* __restrict__ work, size_t work_stride,
                                                                     int32_t* __restrict__ selected, int reuse, int K,
                                                                     float coef, float* __restrict__ loss,
                                                                     float* __restrict__ entropy, int want_grad, int V,
                                                                     int C) {
  __shared__ float s_H[TPT_MAX_V], s_m[TPT_MAX_V], s_sum[TPT_MAX_V];
  __shared__ int s_flag[TPT_MAX_V], s_list[TPT_MAX_V];
  __shared__ float red[TPT_RED_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = TPT_RED_THREADS / 64;
  const int img = blockIdx.x;
  const float* z = work + (size_t)img * work_stride;
  float* dz = work + (size_t)img * work_stride + (size_t)V * C;
  float* g = dz + (size_t)V * C;

  // 1. per view: max, sum of exp(z - max), entropy = log(sum) - sum(e t) / sum with t = z - max <= 0: two terms of one
  //    sign, no cancellation for a confident view.  Every wave runs the same code: H does not depend on the view index.
  for (int v = wave; v < V; v += NW) {
    const float* zr = z + (size_t)v * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, zr[c]);
    m = wave_max(m);
    float ssum = 0.f, a = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float t = zr[c] - m, e = expf(t);
      ssum += e;
      a += e * t;
    }
    ssum = wave_sum(ssum);
    a = wave_sum(a);
    if (lane == 0) {
      const float H = logf(ssum) - a / ssum;
      s_m[v] = m;
      s_sum[v] = ssum;
      s_H[v] = H;
      if (entropy) entropy[(size_t)img * V + v] = H;
    }
  }
  __syncthreads();

  // 2. selection by rank counting (V <= 1024 = the workgroup: thread v owns view v); s_list = the set, ascending
  if (!reuse) {
    int flag = 0;
    if (tid < V) {
      const float Hv = s_H[tid];
      int rank = 0;
      for (int u = 0; u < V; ++u) {
        const float Hu = s_H[u];
        rank += (Hu < Hv || (Hu == Hv && u < tid)) ? 1 : 0;
      }
      flag = rank < K ? 1 : 0;
    }
    s_flag[tid] = flag;
    if (tid < K) s_list[tid] = 0;  // entropies that are not numbers can leave slots unfilled: view 0 then
    __syncthreads();
    if (flag) {
      int pos = 0;
      for (int u = 0; u < tid; ++u) pos += s_flag[u];
      if (pos < K) s_list[pos] = tid;
    }
    __syncthreads();
    if (tid < K) selected[(size_t)img * K + tid] = s_list[tid];
  } else {
    if (tid < K) s_list[tid] = min(max(selected[(size_t)img * K + tid], 0), V - 1);
    __syncthreads();
  }

  // 3. pbar, g = -log pbar (0 where pbar underflowed to 0: the limit of pbar log pbar, and p_v is 0 there too), loss
  float part = 0.f;
  for (int c = tid; c < C; c += TPT_RED_THREADS) {
    float pb = 0.f;
    for (int k = 0; k < K; ++k) {
      const int v = s_list[k];
      pb += expf(z[(size_t)v * C + c] - s_m[v]) / s_sum[v];
    }
    pb = pb / (float)K;
    const float gc = pb > 0.f ? -logf(pb) : 0.f;
    g[c] = gc;
    part += pb * gc;
  }
  part = tpt_block_sum(part, red, tid);  // its barriers also publish g to the workgroup
  if (tid == 0) loss[img] = part;
  if (!want_grad) return;

  // 4. dz rows of the selected views, scaled by coef = grad_scale * s / K
  for (int k = wave; k < K; k += NW) {
    const int v = s_list[k];
    const float* zr = z + (size_t)v * C;
    const float m = s_m[v], ssum = s_sum[v];
    float dot = 0.f;
    for (int c = lane; c < C; c += 64) dot += (expf(zr[c] - m) / ssum) * g[c];
    dot = wave_sum(dot);
    for (int c = lane; c < C; c += 64) dz[(size_t)k * C + c] = coef * ((expf(zr[c] - m) / ssum) * (g[c] - dot));
  }
}

// ------------------------------------------------------------------------------------------------- gradient
// dtext[img, c, :] = sum over k ascending of dz[k, c] F[selected[k], :]
__global__ __launch_bounds__(TPT_THREADS) void tpt_grad_kernel(const float* __restrict__ feats, const float* __restrict__ work,
                                                               size_t work_stride, const int32_t* __restrict__ selected,
                                                               float* __restrict__ dtext, int K, int V, int d, int C) {
  __shared__ int s_sel[TPT_MAX_V];
  const int tid = threadIdx.x, img = blockIdx.y, c0 = blockIdx.x * TPT_GC;
  const float* F = feats + (size_t)img * V * d;
  const float* dz = work + (size_t)img * work_stride + (size_t)V * C;
  for (int k = tid; k < K; k += TPT_THREADS) s_sel[k] = min(max(selected[(size_t)img * K + k], 0), V - 1);
  __syncthreads();
  const int d4 = d >> 2, items = min(TPT_GC, C - c0) * d4;
  for (int it = tid; it < items; it += TPT_THREADS) {
    const int cl = it / d4, j = (it - cl * d4) * 4, c = c0 + cl;
    f32x4 acc;
    acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float wk = dz[(size_t)k * C + c];
      const f32x4 f = *reinterpret_cast<const f32x4*>(F + (size_t)s_sel[k] * d + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(wk, f[e], acc[e]);
    }
    *reinterpret_cast<f32x4*>(dtext + ((size_t)img * C + c) * d + j) = acc;
  }
}

}  // namespace
}  // namespace clipfs

using namespace clipfs;

extern "C" size_t clipfs_tpt_work_floats(int n_img, int views, int width, int classes) {
  (void)width;
  if (n_img < 1 || views < 1 || classes < 1) return 0;
  return (size_t)n_img * (2 * (size_t)views * classes + (size_t)classes);
}

extern "C" int clipfs_tpt_objective(const float* feats, const float* text, int text_per_image, int32_t* selected,
                                    int reuse_selection, int K, float logit_scale, float grad_scale, float* loss,
                                    float* entropy, float* dtext, float* work, int n_img, int views, int width, int classes,
                                    void* stream) {
  CLIPFS_REQUIRE(feats, "tpt_objective: feats is NULL");
  CLIPFS_REQUIRE(text, "tpt_objective: text is NULL");
  CLIPFS_REQUIRE(selected, "tpt_objective: selected is NULL (it is written, or read with reuse_selection)");
  CLIPFS_REQUIRE(loss, "tpt_objective: loss is NULL");
  CLIPFS_REQUIRE(work, "tpt_objective: work is NULL (clipfs_tpt_work_floats floats)");
  CLIPFS_REQUIRE(n_img >= 1 && n_img <= 65535, "tpt_objective: n_img %d outside [1, 65535]", n_img);
  CLIPFS_REQUIRE(views >= 1 && views <= TPT_MAX_V, "tpt_objective: views %d outside [1, %d]", views, TPT_MAX_V);
  CLIPFS_REQUIRE(width >= 4 && width <= TPT_MAX_D && width % 4 == 0,
                 "tpt_objective: width %d must be a multiple of 4 in [4, %d]", width, TPT_MAX_D);
  CLIPFS_REQUIRE(classes >= 1, "tpt_objective: classes %d < 1", classes);
  CLIPFS_REQUIRE(K >= 1 && K <= views, "tpt_objective: K %d outside [1, views = %d]", K, views);
  CLIPFS_REQUIRE(aligned16(feats) && aligned16(text) && aligned16(dtext),
                 "tpt_objective: feats, text and dtext must be 16-byte aligned");
  CLIPFS_REQUIRE(isfinite(logit_scale) && isfinite(grad_scale), "tpt_objective: logit_scale / grad_scale not finite");
  const size_t wstride = 2 * (size_t)views * classes + (size_t)classes;
  const size_t tstride = text_per_image ? (size_t)classes * width : 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tpt_logits_kernel, dim3((classes + 31) / 32, (views + 31) / 32, n_img), dim3(TPT_THREADS), 0, st, feats,
                     text, tstride, work, wstride, views, width, classes, logit_scale);
  hipLaunchKernelGGL(tpt_reduce_kernel, dim3(n_img), dim3(TPT_RED_THREADS), 0, st, work, wstride, selected,
                     reuse_selection ? 1 : 0, K, (logit_scale / (float)K) * grad_scale, loss, entropy, dtext ? 1 : 0, views,
                     classes);
  if (dtext)
    hipLaunchKernelGGL(tpt_grad_kernel, dim3((classes + TPT_GC - 1) / TPT_GC, n_img), dim3(TPT_THREADS), 0, st, feats, work,
                       wstride, selected, dtext, K, views, width, classes);
  return launch_status();
}
