// Token assembly, classifier head, loss, top-k and optimiser kernels (all HBM/latency bound,
// tiny next to the GEMMs; each reads its operands once with 16-byte accesses where rows allow).
#include "common.h"

namespace clipfs {

// ---- ViT special tokens: class row and VPT rows (jclip/model.py:109-114, model1.py:192-194) ----
__global__ __launch_bounds__(256) void vit_fill_special_kernel(float* __restrict__ x, const float* __restrict__ cls,
                                                               const float* __restrict__ pos,
                                                               const float* __restrict__ vpt, int batch, int tokens,
                                                               int n_patch, int n_vpt, int width) {
  const int per_img = (1 + n_vpt) * width;
  const size_t total = (size_t)batch * per_img;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int b = (int)(i / per_img), rem = (int)(i % per_img);
    const int r = rem / width, c = rem % width;
    if (r == 0)
      x[((size_t)b * tokens) * width + c] = cls[c] + pos[c];
    else
      x[((size_t)b * tokens + n_patch + r) * width + c] = vpt[(size_t)(r - 1) * width + c];
  }
}

// ---- text embedding (jclip/model.py:203-205; prompt tokens slow_pace.py:185-199) ----
__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                         const float* __restrict__ pos, const float* __restrict__ ctx,
                                                         int n_ctx, float* __restrict__ x, int n, int seq, int width) {
  const int nch = width >> 2;
  const size_t total = (size_t)n * seq * nch;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % nch);
    const size_t tok = i / nch;
    const int l = (int)(tok % seq);
    const float4* src;
    if (ctx && l >= 1 && l <= n_ctx)
      src = reinterpret_cast<const float4*>(ctx + (size_t)(l - 1) * width);
    else
      src = reinterpret_cast<const float4*>(table + (size_t)ids[tok] * width);
    const float4 e = src[c];
    const float4 pe = reinterpret_cast<const float4*>(pos + (size_t)l * width)[c];
    reinterpret_cast<float4*>(x + tok * width)[c] = make_float4(e.x + pe.x, e.y + pe.y, e.z + pe.z, e.w + pe.w);
  }
}

// dctx[i, :] += sum_c dx[c, first + i, :]
__global__ __launch_bounds__(256) void text_ctx_grad_kernel(const float* __restrict__ dx, float* __restrict__ dctx, int n,
                                                            int seq, int width, int n_ctx, int first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ctx * width) return;
  const int r = i / width, c = i % width;
  float acc = 0.f;
  for (int k = 0; k < n; ++k) acc += dx[((size_t)k * seq + first + r) * width + c];
  dctx[i] += acc;
}

// EOT row = first position of the largest token id (jclip/model.py:213-214)
__global__ __launch_bounds__(64) void gather_eot_kernel(const float* __restrict__ x, const int64_t* __restrict__ ids,
                                                        float* __restrict__ out, int32_t* __restrict__ idx_out, int seq,
                                                        int width) {
  const int c = blockIdx.x, lane = threadIdx.x;
  long long best = -1;
  int besti = 0;
  for (int l = lane; l < seq; l += 64) {
    const long long v = ids[(size_t)c * seq + l];
    if (v > best) {
      best = v;
      besti = l;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(besti, off, 64);
    if (ov > best || (ov == best && oi < besti)) {
      best = ov;
      besti = oi;
    }
  }
  if (idx_out && lane == 0) idx_out[c] = besti;
  const float* src = x + ((size_t)c * seq + besti) * width;
  for (int k = lane; k < width; k += 64) out[(size_t)c * width + k] = src[k];
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ dy, const int32_t* __restrict__ idx,
                                                           float* __restrict__ dx, int n, int seq, int width) {
  const size_t total = (size_t)n * seq * width;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % width);
    const size_t tok = i / width;
    const int c = (int)(tok / seq), l = (int)(tok % seq);
    dx[i] = (l == idx[c]) ? dy[(size_t)c * width + k] : 0.f;
  }
}

// out[c, :] = src[(c * seq + idx[c]) * ld + 0..width)  -- one row per sequence (the class token / the EOT token)
__global__ __launch_bounds__(256) void gather_seq_rows_kernel(const float* __restrict__ src, size_t ld,
                                                              const int32_t* __restrict__ idx, float* __restrict__ out,
                                                              int n, int seq, int width) {
  const size_t total = (size_t)n * width;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % width), c = (int)(i / width);
    out[i] = src[((size_t)c * seq + idx[c]) * ld + k];
  }
}

// dx[(c * seq + idx[c]) * width + k] += src[c, k]
__global__ __launch_bounds__(256) void add_seq_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                           float* __restrict__ dx, int n, int seq, int width) {
  const size_t total = (size_t)n * width;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % width), c = (int)(i / width);
    dx[((size_t)c * seq + idx[c]) * width + k] += src[i];
  }
}

// dst[(c * seq + idx[c]) * ld + k] = src[c, k]   (the other rows are left alone)
__global__ __launch_bounds__(256) void put_seq_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                           float* __restrict__ dst, size_t ld, int n, int seq, int width) {
  const size_t total = (size_t)n * width;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % width), c = (int)(i / width);
    dst[((size_t)c * seq + idx[c]) * ld + k] = src[i];
  }
}

// packed rows (the text tower's live-row backward): out[i, :] = src[map[i] * ld + 0..width) and its inverse
// dst[map[i] * ld + 0..width) = src[i, :]; V = 4 moves float4 (width, ld and both bases 16-byte multiples)
template <int V>
__global__ __launch_bounds__(256) void gather_rows_map_kernel(const float* __restrict__ src, size_t ld, const int32_t* __restrict__ map,
                                                              float* __restrict__ out, int n, int width) {
  typedef float vec __attribute__((ext_vector_type(V)));
  const int wv = width / V;
  const size_t total = (size_t)n * wv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % wv), r = (int)(i / wv);
    reinterpret_cast<vec*>(out)[i] = *reinterpret_cast<const vec*>(src + (size_t)map[r] * ld + (size_t)k * V);
  }
}
template <int V>
__global__ __launch_bounds__(256) void put_rows_map_kernel(const float* __restrict__ src, const int32_t* __restrict__ map,
                                                           float* __restrict__ dst, size_t ld, int n, int width) {
  typedef float vec __attribute__((ext_vector_type(V)));
  const int wv = width / V;
  const size_t total = (size_t)n * wv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % wv), r = (int)(i / wv);
    *reinterpret_cast<vec*>(dst + (size_t)map[r] * ld + (size_t)k * V) = reinterpret_cast<const vec*>(src)[i];
  }
}

// the same two for a tensor stored as f16 (fp16 storage mode: the saved pre-GELU activation); the compact side stays fp32
__global__ __launch_bounds__(256) void gather_seq_rows_f16_kernel(const _Float16* __restrict__ src, size_t ld,
                                                                  const int32_t* __restrict__ idx, float* __restrict__ out,
                                                                  int n, int seq, int width) {
  const size_t total = (size_t)n * width;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % width), c = (int)(i / width);
    out[i] = (float)src[((size_t)c * seq + idx[c]) * ld + k];
  }
}
__global__ __launch_bounds__(256) void put_seq_rows_f16_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                               _Float16* __restrict__ dst, size_t ld, int n, int seq, int width) {
  const size_t total = (size_t)n * width;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % width), c = (int)(i / width);
    dst[((size_t)c * seq + idx[c]) * ld + k] = (_Float16)src[i];
  }
}

// idx[c] = argmax_l ids[c, l] (first maximum: the EOT token has the largest id, jclip/model.py:213-214)
__global__ __launch_bounds__(64) void eot_index_kernel(const int64_t* __restrict__ ids, int32_t* __restrict__ idx, int n, int seq) {
  const int c = blockIdx.x, lane = threadIdx.x;
  long best = -1;
  int at = 0;
  for (int l = lane; l < seq; l += 64) {
    const long v = ids[(size_t)c * seq + l];
    if (v > best) {
      best = v;
      at = l;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const long ob = __shfl_xor(best, off, 64);
    const int oa = __shfl_xor(at, off, 64);
    if (ob > best || (ob == best && oa < at)) {
      best = ob;
      at = oa;
    }
  }
  if (lane == 0) idx[c] = at;
}

// ---- per class: normalise templates, mean, normalise (lora_train_vlp.py:978-990) ----  one wave per class
__global__ __launch_bounds__(64) void class_mean_fwd_kernel(const float* __restrict__ emb, float* __restrict__ out,
                                                            int templates, int width) {
  const int c = blockIdx.x, lane = threadIdx.x;
  constexpr int MAXW = 32;  // width <= 2048
  float acc[MAXW];
#pragma unroll
  for (int i = 0; i < MAXW; ++i) acc[i] = 0.f;
  for (int t = 0; t < templates; ++t) {
    const float* e = emb + ((size_t)c * templates + t) * width;
    float v[MAXW];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXW; ++i) {
      const int k = lane + 64 * i;
      v[i] = k < width ? e[k] : 0.f;
      s = fmaf(v[i], v[i], s);
    }
    const float nrm = sqrtf(wave_sum(s));
#pragma unroll
    for (int i = 0; i < MAXW; ++i) acc[i] += v[i] / nrm;
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXW; ++i) {
    acc[i] = acc[i] / (float)templates;
    s = fmaf(acc[i], acc[i], s);
  }
  const float nrm = sqrtf(wave_sum(s));
#pragma unroll
  for (int i = 0; i < MAXW; ++i) {
    const int k = lane + 64 * i;
    if (k < width) out[(size_t)c * width + k] = acc[i] / nrm;
  }
}

// backward of class_mean_fwd: demb from dout, recomputing the normalised templates.  one wave per class
__global__ __launch_bounds__(64) void class_mean_bwd_kernel(const float* __restrict__ emb, const float* __restrict__ dout,
                                                            float* __restrict__ demb, int templates, int width) {
  const int c = blockIdx.x, lane = threadIdx.x;
  constexpr int MAXW = 32;
  float acc[MAXW];
#pragma unroll
  for (int i = 0; i < MAXW; ++i) acc[i] = 0.f;
  for (int t = 0; t < templates; ++t) {
    const float* e = emb + ((size_t)c * templates + t) * width;
    float v[MAXW];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXW; ++i) {
      const int k = lane + 64 * i;
      v[i] = k < width ? e[k] : 0.f;
      s = fmaf(v[i], v[i], s);
    }
    const float nrm = sqrtf(wave_sum(s));
#pragma unroll
    for (int i = 0; i < MAXW; ++i) acc[i] += v[i] / nrm;
  }
  // m = acc / T ; out = m / |m| ; dm = (dout - out <dout, out>) / |m| ; each template gets dm / T
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXW; ++i) {
    acc[i] = acc[i] / (float)templates;
    s = fmaf(acc[i], acc[i], s);
  }
  const float mn = sqrtf(wave_sum(s));
  float g[MAXW];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < MAXW; ++i) {
    const int k = lane + 64 * i;
    g[i] = k < width ? dout[(size_t)c * width + k] : 0.f;
    dot = fmaf(g[i], acc[i] / mn, dot);
  }
  dot = wave_sum(dot);
#pragma unroll
  for (int i = 0; i < MAXW; ++i) g[i] = (g[i] - (acc[i] / mn) * dot) / (mn * (float)templates);
  for (int t = 0; t < templates; ++t) {
    const float* e = emb + ((size_t)c * templates + t) * width;
    float v[MAXW];
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXW; ++i) {
      const int k = lane + 64 * i;
      v[i] = k < width ? e[k] : 0.f;
      s2 = fmaf(v[i], v[i], s2);
    }
    const float nrm = sqrtf(wave_sum(s2));
    float d2 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXW; ++i) d2 = fmaf(g[i], v[i] / nrm, d2);
    d2 = wave_sum(d2);
#pragma unroll
    for (int i = 0; i < MAXW; ++i) {
      const int k = lane + 64 * i;
      if (k < width) demb[((size_t)c * templates + t) * width + k] = (g[i] - (v[i] / nrm) * d2) / nrm;
    }
  }
}

// ---- softmax cross entropy, one wave per row (lora_train_vlp.py:997) ----
__device__ __forceinline__ void cross_entropy_rows(const float* __restrict__ logits,
                                                   const int64_t* __restrict__ target,
                                                   float* __restrict__ dlogits, float* __restrict__ loss_rows,
                                                   int32_t* __restrict__ correct_rows, int rows, int classes,
                                                   float grad_scale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* z = logits + (size_t)row * classes;
  float m = -INFINITY;
  int am = 0;
  for (int k = lane; k < classes; k += 64) {
    const float v = z[k];
    if (v > m) {
      m = v;
      am = k;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(m, off, 64);
    const int oi = __shfl_xor(am, off, 64);
    if (ov > m || (ov == m && oi < am)) {
      m = ov;
      am = oi;
    }
  }
  float s = 0.f;
  for (int k = lane; k < classes; k += 64) s += __expf(z[k] - m);
  s = wave_sum(s);
  const int tgt = (int)target[row];
  const float lse = __logf(s);
  if (lane == 0) {
    loss_rows[row] = lse - (z[tgt] - m);
    if (correct_rows) correct_rows[row] = (am == tgt) ? 1 : 0;
  }
  if (dlogits) {
    const float inv = grad_scale / ((float)rows * s);
    for (int k = lane; k < classes; k += 64) {
      float gk = __expf(z[k] - m) * inv;
      if (k == tgt) gk -= grad_scale / (float)rows;
      dlogits[(size_t)row * classes + k] = gk;
    }
  }
}
// state = a scaler record (clipfs.h: "loss scaling") whose loss scale is folded into the gradient scale, or NULL; the
// per-row losses and hit flags do not depend on it
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float* __restrict__ logits,
                                                            const int64_t* __restrict__ target,
                                                            float* __restrict__ dlogits, float* __restrict__ loss_rows,
                                                            int32_t* __restrict__ correct_rows, int rows, int classes,
                                                            float grad_scale, const float* __restrict__ state) {
  cross_entropy_rows(logits, target, dlogits, loss_rows, correct_rows, rows, classes,
                     state ? grad_scale * state[CLIPFS_SCALER_SCALE] : grad_scale);
}

// deterministic final reduction of the per-row losses / hit flags (single wave, fixed order)
__global__ __launch_bounds__(64) void ce_finish_kernel(const float* __restrict__ loss_rows,
                                                       const int32_t* __restrict__ correct_rows,
                                                       float* __restrict__ loss_sum, int32_t* __restrict__ correct,
                                                       int rows) {
  const int lane = threadIdx.x;
  float s = 0.f;
  int c = 0;
  for (int r = lane; r < rows; r += 64) {
    s += loss_rows[r];
    if (correct_rows) c += correct_rows[r];
  }
  s = wave_sum(s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if (lane == 0) {
    loss_sum[0] = s;
    if (correct) correct[0] = c;
  }
}

// ---- top-k (k <= 8): repeated arg-max with ties to the smaller index, one wave per row ----
__global__ __launch_bounds__(64) void topk_kernel(const float* __restrict__ logits, int32_t* __restrict__ labels,
                                                  int classes, int k) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* z = logits + (size_t)row * classes;
  float prev_v = INFINITY;
  int prev_i = -1;
  for (int t = 0; t < k; ++t) {
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < classes; c += 64) {
      const float v = z[c];
      // candidates strictly after the previous pick in (value desc, index asc) order
      const bool after = (v < prev_v) || (v == prev_v && c > prev_i);
      if (after && (v > m || (v == m && c < am))) {
        m = v;
        am = c;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(m, off, 64);
      const int oi = __shfl_xor(am, off, 64);
      if (ov > m || (ov == m && oi < am)) {
        m = ov;
        am = oi;
      }
    }
    if (lane == 0) labels[(size_t)row * k + t] = am;
    prev_v = m;
    prev_i = am;
  }
}

// ---- Channel_LP affine (slow_pace.py:1195-1206) and logit_normalize (:1276-1280) ----
__global__ __launch_bounds__(256) void channel_affine_kernel(const float* __restrict__ x, const float* __restrict__ s1,
                                                             const float* __restrict__ b1, float* __restrict__ y,
                                                             size_t total, int width) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % width);
    y[i] = s1[c] * x[i] + b1[c];
  }
}

// single workgroup: global mean / unbiased std (clamped) over all elements, then per-row centring
__global__ __launch_bounds__(1024) void logit_normalize_kernel(const float* __restrict__ z, float* __restrict__ out,
                                                               float* __restrict__ work, int rows, int classes) {
  __shared__ float red[16];
  __shared__ float stat[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = (size_t)rows * classes;
  float s = 0.f;
  for (size_t i = tid; i < n; i += 1024) s += z[i];
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    stat[0] = t / (float)n;
  }
  __syncthreads();
  const float mean = stat[0];
  float q = 0.f;
  for (size_t i = tid; i < n; i += 1024) {
    const float d = z[i] - mean;
    q = fmaf(d, d, q);
  }
  q = wave_sum(q);
  __syncthreads();
  if (lane == 0) red[wave] = q;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    stat[1] = sqrtf(fmaxf(t / (float)(n - 1), 1e-6f));
    if (work) {
      work[0] = mean;
      work[1] = stat[1];
    }
  }
  __syncthreads();
  const float sd = stat[1];
  for (int r = wave; r < rows; r += 16) {
    float rs = 0.f;
    for (int c = lane; c < classes; c += 64) rs += z[(size_t)r * classes + c];
    const float rm = wave_sum(rs) / (float)classes;
    for (int c = lane; c < classes; c += 64) out[(size_t)r * classes + c] = (z[(size_t)r * classes + c] - rm) / sd;
  }
}

// backward of logit_normalize: zn = (z - rowmean(z)) / sigma, sigma = sqrt(max(sum((z - mean_all)^2)/(n-1), 1e-6))
//   dz = (dzn - rowmean(dzn)) / sigma  -  (sum(dzn * zn) / sigma) * (z - mean_all) / ((n - 1) * sigma)   [2nd term 0 if clamped]
__global__ __launch_bounds__(1024) void logit_normalize_bwd_kernel(const float* __restrict__ z,
                                                                   const float* __restrict__ dzn, float* __restrict__ dz,
                                                                   int rows, int classes) {
  __shared__ float red[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = (size_t)rows * classes;
  auto block_total = [&](float v) -> float {
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    return t;
  };
  // every mean is taken of z - z[0]: a sum of logits that all sit near 300 rounds to an ulp of n * 300, and the centred
  // values it leaves behind carry that error at full size
  const float z0 = z[0];
  float s = 0.f;
  for (size_t i = tid; i < n; i += 1024) s += z[i] - z0;
  const float mean = block_total(s) / (float)n;  // of z - z0
  float q = 0.f;
  for (size_t i = tid; i < n; i += 1024) {
    const float d = (z[i] - z0) - mean;
    q = fmaf(d, d, q);
  }
  const float var = block_total(q) / (float)(n - 1);
  const bool clamped = var < 1e-6f;
  const float sd = sqrtf(fmaxf(var, 1e-6f));
  // g = sum_ij dzn_ij * (z_ij - rowmean_i) ; needs the row means first: each wave owns rows r = wave, wave+16, ...
  float g = 0.f;
  for (int r = wave; r < rows; r += 16) {
    float rs = 0.f;
    for (int c = lane; c < classes; c += 64) rs += z[(size_t)r * classes + c] - z0;
    const float rm = wave_sum(rs) / (float)classes;  // of z - z0
    for (int c = lane; c < classes; c += 64) g = fmaf(dzn[(size_t)r * classes + c], (z[(size_t)r * classes + c] - z0) - rm, g);
  }
  g = block_total(g);  // = sigma * sum(dzn * zn)
  const float coef = clamped ? 0.f : g / (sd * sd * sd * (float)(n - 1));
  for (int r = wave; r < rows; r += 16) {
    float ds = 0.f;
    for (int c = lane; c < classes; c += 64) ds += dzn[(size_t)r * classes + c];
    const float dm = wave_sum(ds) / (float)classes;
    for (int c = lane; c < classes; c += 64) {
      const size_t i = (size_t)r * classes + c;
      dz[i] = (dzn[i] - dm) / sd - coef * ((z[i] - z0) - mean);
    }
  }
}

// out[c] (+)= sum_r x[r,c] * (y ? y[r,c] : 1)     one thread per column, fixed row order
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                     float* __restrict__ out, int rows, int cols) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float acc = 0.f;
  for (int r = 0; r < rows; ++r) {
    const float v = x[(size_t)r * cols + c];
    acc = y ? fmaf(v, y[(size_t)r * cols + c], acc) : acc + v;
  }
  out[c] = acc;
}

// ---- AdamW over the flat trainable buffer (lora_train_vlp.py:946,1002) ----
__device__ __forceinline__ void adamw_element(float* __restrict__ p, const float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v, size_t i, float lr,
                                              float b1, float b2, float eps, float wd, float inv_sqrt_bc2,
                                              float step_size, float grad_scale) {
  const float gi = g[i] * grad_scale;
  float pi = p[i] * (1.f - lr * wd);
  const float mi = b1 * m[i] + (1.f - b1) * gi;
  const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
  const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
  pi -= step_size * mi / denom;
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
}
// The one AdamW kernel, with three optional records (each NULL or given, uniform over the launch): bias corrections,
// gradient scale and the skip decision from the loss-scaling record sf when there is one (below), the gradient
// multiplier from the clip record cs when there is one, and the EMA shadow updated from the parameter just computed.
// With all three NULL it is the plain update at the arguments' inv_sqrt_bc2 / step_size / grad_scale.  Elements from
// tail_start on (n: none) take the decay tail_wd and are clamped to [tail_min, tail_max] before the shadow reads them.
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                                                    float b1, float b2, float eps, float wd, float inv_sqrt_bc2,
                                                    float step_size, float grad_scale,
                                                    const float* __restrict__ sf, const float* __restrict__ cs,
                                                    float* __restrict__ shadow, float decay, float one_minus_decay,
                                                    size_t tail_start, float tail_wd, float tail_min, float tail_max) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (sf) {
    if (reinterpret_cast<const int32_t*>(sf)[CLIPFS_SCALER_SKIP] != 0) return;
    inv_sqrt_bc2 = sf[CLIPFS_SCALER_INV_SQRT_BC2];
    step_size = sf[CLIPFS_SCALER_STEP_SIZE];
    grad_scale = sf[CLIPFS_SCALER_INV_SCALE];
  }
  if (cs) grad_scale = cs[CLIPFS_CLIP_MULT];
  const bool tail = i >= tail_start;
  adamw_element(p, g, m, v, i, lr, b1, b2, eps, tail ? tail_wd : wd, inv_sqrt_bc2, step_size, grad_scale);
  if (tail) p[i] = fminf(fmaxf(p[i], tail_min), tail_max);
  if (shadow) shadow[i] = fmaf(decay, shadow[i], one_minus_decay * p[i]);
}

// ---- loss scaling for f16 gradient storage: the scaler record is CLIPFS_SCALER_WORDS 32-bit words (clipfs.h) ----
// One pass over the flat gradient buffer: a lane that meets NaN or +-inf (exponent field all ones) stores 1 to the
// record's flag.  Every writer stores the same value: no atomics.  Up to 3 floats before the first 16-byte boundary
// and up to 3 after the last whole float4 are read one by one by the first threads of block 0.
__global__ __launch_bounds__(256) void grads_nonfinite_kernel(const float* __restrict__ g, size_t n, unsigned head,
                                                              int32_t* __restrict__ state) {
  const size_t nvec = (n - head) >> 2;
  const unsigned tail = (unsigned)((n - head) & 3);
  const uint4* gv = reinterpret_cast<const uint4*>(g + head);
  unsigned bad = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    const uint4 w = gv[i];
    bad |= (unsigned)((w.x & 0x7f800000u) == 0x7f800000u) | (unsigned)((w.y & 0x7f800000u) == 0x7f800000u) |
           (unsigned)((w.z & 0x7f800000u) == 0x7f800000u) | (unsigned)((w.w & 0x7f800000u) == 0x7f800000u);
  }
  if (blockIdx.x == 0 && threadIdx.x < head + tail) {
    const size_t i = threadIdx.x < head ? (size_t)threadIdx.x : (size_t)head + 4 * nvec + (threadIdx.x - head);
    bad |= (unsigned)((__float_as_uint(g[i]) & 0x7f800000u) == 0x7f800000u);
  }
  if (bad) state[CLIPFS_SCALER_FOUND] = 1;
}

// One thread: turn the flag into this step's decision and the next step's scale.
__global__ __launch_bounds__(64) void scaler_decide_kernel(float* __restrict__ sf, float lr, float b1, float b2,
                                                           float growth_factor, float backoff_factor,
                                                           int growth_interval) {
  if (threadIdx.x != 0) return;
  int32_t* si = reinterpret_cast<int32_t*>(sf);
  const float scale = sf[CLIPFS_SCALER_SCALE];
  sf[CLIPFS_SCALER_INV_SCALE] = 1.f / scale;  // of the scale THIS step's gradients carry
  if (si[CLIPFS_SCALER_FOUND] == 0) {
    const int step = si[CLIPFS_SCALER_STEP] + 1;
    si[CLIPFS_SCALER_STEP] = step;
    const double bc1 = 1.0 - pow((double)b1, (double)step);
    const double bc2 = 1.0 - pow((double)b2, (double)step);
    sf[CLIPFS_SCALER_INV_SQRT_BC2] = (float)(1.0 / sqrt(bc2));
    sf[CLIPFS_SCALER_STEP_SIZE] = (float)((double)lr / bc1);
    si[CLIPFS_SCALER_SKIP] = 0;
    int tracker = si[CLIPFS_SCALER_TRACKER] + 1;
    if (growth_interval > 0 && tracker >= growth_interval) {
      const float grown = scale * growth_factor;
      if (grown <= 3.402823466e38f) sf[CLIPFS_SCALER_SCALE] = grown;  // a scale that would overflow stays
      tracker = 0;
    }
    si[CLIPFS_SCALER_TRACKER] = tracker;
  } else {
    si[CLIPFS_SCALER_SKIPPED] += 1;
    si[CLIPFS_SCALER_SKIP] = 1;
    sf[CLIPFS_SCALER_SCALE] = scale * backoff_factor;
    si[CLIPFS_SCALER_TRACKER] = 0;
  }
  si[CLIPFS_SCALER_FOUND] = 0;
}

// ---- gradient clipping by global norm + EMA shadow (clipfs.h: "optimiser step options") ----
// Sum of squares of the flat gradient, two launches, no float atomics.  The buffer is cut into `chunks` runs of `cpe`
// elements (both functions of n alone, cpe a multiple of 4); workgroup b owns elements [b * cpe, min(n, (b + 1) * cpe)).
// Every run starts at the same offset from a 16-byte boundary as the buffer does, so each workgroup reads its up to 3
// floats before the first boundary and up to 3 after the last whole float4 one by one and everything between with
// 16-byte loads; nothing outside [0, n) is touched.  The square of an fp32 value is exact in double and so is its
// range: 1e19^2 * n stays far below DBL_MAX.
constexpr size_t kSumsqMinChunk = 4096;  // elements per workgroup at least: 256 threads x 4 float4
constexpr size_t kSumsqMaxChunks = 512;  // partials the decision's single lane adds

static inline size_t sumsq_chunks(size_t n) {
  if (n == 0) return 0;
  const size_t c = (n + kSumsqMinChunk - 1) / kSumsqMinChunk;
  return c < kSumsqMaxChunks ? c : kSumsqMaxChunks;
}
static inline size_t sumsq_chunk_elems(size_t n) {  // multiple of 4, >= kSumsqMinChunk for n > 0
  const size_t chunks = sumsq_chunks(n);
  const size_t cpe = chunks == kSumsqMaxChunks ? (n + chunks - 1) / chunks : kSumsqMinChunk;
  return (cpe + 3) & ~(size_t)3;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, size_t cpe,
                                                         unsigned head_of_base, double* __restrict__ work) {
  const size_t e0 = (size_t)blockIdx.x * cpe;
  if (e0 >= n) {  // uniform over the workgroup; sumsq_chunk_elems leaves no run empty, but the partial stays defined
    if (threadIdx.x == 0) work[blockIdx.x] = 0.0;
    return;
  }
  const size_t len = (n - e0 < cpe) ? n - e0 : cpe;
  const unsigned head = head_of_base < len ? head_of_base : (unsigned)len;
  const size_t nvec = (len - head) >> 2;
  const unsigned tail = (unsigned)((len - head) & 3);
  const float* gb = g + e0;
  const float4* gv = reinterpret_cast<const float4*>(gb + head);
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < nvec; i += 256) {
    const float4 w = gv[i];
    acc += (double)w.x * (double)w.x;
    acc += (double)w.y * (double)w.y;
    acc += (double)w.z * (double)w.z;
    acc += (double)w.w * (double)w.w;
  }
  if (threadIdx.x < head + tail) {
    const size_t i = threadIdx.x < head ? (size_t)threadIdx.x : (size_t)head + 4 * nvec + (threadIdx.x - head);
    const double x = (double)gb[i];
    acc += x * x;
  }
  __shared__ double red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {  // fixed tree: thread t adds slot t + s
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) work[blockIdx.x] = red[0];
}

// One workgroup: the partials go through LDS, lane 0 adds them in index order and writes the clip record with
// ordinary vector stores.  sf = the loss-scaling record (after scaler_decide: INV_SCALE is the scale these gradients
// carry) or NULL.
__global__ __launch_bounds__(256) void clip_decide_kernel(const double* __restrict__ work, int chunks, float max_norm,
                                                          const float* __restrict__ sf, float* __restrict__ cs) {
  __shared__ double part[kSumsqMaxChunks];
  for (int k = threadIdx.x; k < chunks; k += 256) part[k] = work[k];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int k = 0; k < chunks; ++k) total += part[k];
  const float inv_scale = sf ? sf[CLIPFS_SCALER_INV_SCALE] : 1.f;
  const float norm = (float)(sqrt(total) * (double)inv_scale);
  float coef = 0.f;  // a NaN or infinite norm
  if (norm <= 3.402823466e38f) {
    const double c = (double)max_norm / ((double)norm + 1e-6);
    coef = c < 1.0 ? (float)c : 1.f;
  }
  cs[CLIPFS_CLIP_NORM] = norm;
  cs[CLIPFS_CLIP_COEF] = coef;
  cs[CLIPFS_CLIP_MULT] = inv_scale * coef;
}

// C[m,n] = alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn]   (tiny products whose reduction dim is
// not 16-byte friendly, e.g. over the 403 classes in the logits backward)
__global__ __launch_bounds__(256) void matmul_small_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                           float* __restrict__ C, int M, int N, int K, long sam, long sak,
                                                           long sbk, long sbn, float alpha) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(A[m * sam + k * sak], B[k * sbk + n * sbn], acc);
  C[i] = alpha * acc;
}

static inline unsigned grid_for(size_t total) {
  size_t b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}


// ---- stage-2 self-consistency losses (slow_pace.py:1653-1658, kl_div :1170-1177) ----------------------------------
// L1: loss = mean |a - b| ; da = sign(a - b) * grad_scale / n.  One 1024-thread block: fixed thread -> element
// assignment and a fixed LDS tree, so the sum is bitwise reproducible (n is a few 1e5 on the path).
__global__ __launch_bounds__(1024) void l1_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                       float* __restrict__ loss, float* __restrict__ da, float gscale) {
  __shared__ float red[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float g = gscale / (float)n;
  float acc = 0.f;
  for (size_t i = threadIdx.x; i < n; i += 1024) {
    const float d = a[i] - b[i];
    acc += fabsf(d);
    if (da) da[i] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
  }
  acc = wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    loss[0] = t / (float)n;
  }
}

// KL(softmax(t) || softmax(x)) per row:  loss_rows[r] = sum_j q_j (log q_j - log p_j),  dx = (p - q) * grad_scale.
// One wave per row (403 classes); both log-softmaxes with max subtraction, and the maximum subtracted FIRST: log p =
// (x - max) - log(sum), never x - (max + log(sum)), which rounds log(sum) to an ulp of the maximum (3e-5 at logits of
// 300) and shifts every log p of the row by it.  exp / log are the precise ones: q (b - a) multiplies q's error by
// log-ratios of a hundred and more.
__global__ __launch_bounds__(256) void kl_logits_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                        float* __restrict__ loss_rows, float* __restrict__ dx, int rows,
                                                        int cols, float gscale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * cols;
  const float* tr = t + (size_t)row * cols;
  float mx = -INFINITY, mt = -INFINITY;
  for (int j = lane; j < cols; j += 64) {
    mx = fmaxf(mx, xr[j]);
    mt = fmaxf(mt, tr[j]);
  }
  mx = wave_max(mx);
  mt = wave_max(mt);
  float sx = 0.f, st = 0.f;
  for (int j = lane; j < cols; j += 64) {
    sx += expf(xr[j] - mx);
    st += expf(tr[j] - mt);
  }
  sx = wave_sum(sx);
  st = wave_sum(st);
  const float lsx = logf(sx), lst = logf(st);
  float acc = 0.f;
  for (int j = lane; j < cols; j += 64) {
    const float a = (xr[j] - mx) - lsx, b = (tr[j] - mt) - lst;  // log p, log q
    const float q = expf(b);
    acc += q * (b - a);
    if (dx) dx[(size_t)row * cols + j] = (expf(a) - q) * gscale;
  }
  acc = wave_sum(acc);
  if (lane == 0) loss_rows[row] = acc;
}

// ---- the stage-2 objective without its head branch, in one launch (slow_pace.py:1640,1650-1658,1684-1686) ----------
// A wave per row over three kinds of rows: B logits rows (cross entropy of cos + KL against the zero-shot logits), then
// B image-feature rows and n_loc text-feature rows (L1 against the zero-shot features).  V = 4 moves float4 (the host
// checked that the row width and every base of that kind are 16-byte multiples).  Every row leaves one partial per term
// in `work`; stage2_finish_kernel adds them in a fixed order.  `state` (may be NULL) is a loss-scaling record: the three
// gradient outputs carry its scale as their LAST multiplication, so a power-of-two scale changes exponents only.
template <int V>
__device__ __forceinline__ void s2_load(const float* __restrict__ p, int k, float (&v)[4]) {
  if (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + k);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = p[k];
  }
}
template <int V>
__device__ __forceinline__ void s2_store(float* __restrict__ p, int k, const float (&v)[4]) {
  if (V == 4)
    *reinterpret_cast<float4*>(p + k) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[k] = v[0];
}

template <int V>
__device__ __forceinline__ void s2_logits_row(const float* __restrict__ x, const float* __restrict__ t, int tgt,
                                              float* __restrict__ dx, int n, float inv_bg, float inv_bgc, float S,
                                              int lane, float* __restrict__ ce_out, float* __restrict__ kl_out,
                                              int32_t* __restrict__ hit_out) {
  float mx = -INFINITY, mt = -INFINITY;
  int am = 0x7fffffff;
  for (int k = lane * V; k < n; k += 64 * V) {
    float a[4], b[4];
    s2_load<V>(x, k, a);
    s2_load<V>(t, k, b);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (a[e] > mx) {
        mx = a[e];
        am = k + e;
      }
      mt = fmaxf(mt, b[e]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {  // arg-max with ties to the smaller index (clipfs_cross_entropy's rule)
    const float ov = __shfl_xor(mx, off, 64);
    const int oi = __shfl_xor(am, off, 64);
    if (ov > mx || (ov == mx && oi < am)) {
      mx = ov;
      am = oi;
    }
  }
  mt = wave_max(mt);
  float sx = 0.f, st = 0.f;
  for (int k = lane * V; k < n; k += 64 * V) {
    float a[4], b[4];
    s2_load<V>(x, k, a);
    s2_load<V>(t, k, b);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      sx += __expf(a[e] - mx);
      st += __expf(b[e] - mt);
    }
  }
  sx = wave_sum(sx);
  st = wave_sum(st);
  const float lx = mx + __logf(sx), lt = mt + __logf(st);
  const bool tgt_ok = tgt >= 0 && tgt < n;  // a label outside [0, C) reads nothing: its row's loss is NaN
  float kl = 0.f;
  for (int k = lane * V; k < n; k += 64 * V) {
    float a[4], b[4], g[4];
    s2_load<V>(x, k, a);
    s2_load<V>(t, k, b);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float la = a[e] - lx, lb = b[e] - lt;  // log p, log q
      const float p = __expf(la), q = __expf(lb);
      kl += q * (lb - la);
      const float ce = (p - ((k + e) == tgt ? 1.f : 0.f)) * inv_bg;
      g[e] = S * (ce + (p - q) * inv_bgc);
    }
    if (dx) s2_store<V>(dx, k, g);
  }
  kl = wave_sum(kl);
  if (lane == 0) {
    *ce_out = tgt_ok ? lx - x[tgt] : NAN;
    *kl_out = kl;
    *hit_out = (tgt_ok && am == tgt) ? 1 : 0;
  }
}

template <int V>
__device__ __forceinline__ void s2_l1_row(const float* __restrict__ a, const float* __restrict__ b,
                                          float* __restrict__ da, int n, float g, int lane, float* __restrict__ out) {
  float acc = 0.f;
  for (int k = lane * V; k < n; k += 64 * V) {
    float u[4], w[4], s[4];
    s2_load<V>(a, k, u);
    s2_load<V>(b, k, w);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float d = u[e] - w[e];
      acc += fabsf(d);
      s[e] = d > 0.f ? g : (d < 0.f ? -g : 0.f);  // sign(0) = 0, as l1_loss_kernel
    }
    if (da) s2_store<V>(da, k, s);
  }
  acc = wave_sum(acc);
  if (lane == 0) *out = acc;
}

__global__ __launch_bounds__(256) void stage2_objective_kernel(
    const float* __restrict__ cosl, const float* __restrict__ zsl, const int64_t* __restrict__ target,
    const float* __restrict__ img, const float* __restrict__ zs_img, const float* __restrict__ txt,
    const float* __restrict__ zs_txt, float* __restrict__ dcos, float* __restrict__ dimg, float* __restrict__ dtxt,
    float* __restrict__ work, int B, int C, int d, int n_loc, float inv_bg, const float* __restrict__ state, int vec_c,
    int vec_d) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * B + n_loc) return;
  const float S = state ? state[CLIPFS_SCALER_SCALE] : 1.f;
  int32_t* hits = reinterpret_cast<int32_t*>(work + 3 * (size_t)B + n_loc);
  if (row < B) {
    const size_t o = (size_t)row * C;
    const int tgt = (int)target[row];
    float* dx = dcos ? dcos + o : nullptr;
    const float inv_bgc = inv_bg / (float)C;
    if (vec_c)
      s2_logits_row<4>(cosl + o, zsl + o, tgt, dx, C, inv_bg, inv_bgc, S, lane, work + row, work + B + row, hits + row);
    else
      s2_logits_row<1>(cosl + o, zsl + o, tgt, dx, C, inv_bg, inv_bgc, S, lane, work + row, work + B + row, hits + row);
  } else {
    const bool image = row < 2 * B;
    const int r = image ? row - B : row - 2 * B;
    const size_t o = (size_t)r * d;
    const float* a = (image ? img : txt) + o;
    const float* b = (image ? zs_img : zs_txt) + o;
    float* dst = image ? dimg : dtxt;
    float* da = dst ? dst + o : nullptr;
    const float g = S * (image ? inv_bg / (float)d : 1.f / ((float)C * (float)d));
    float* out = work + 2 * (size_t)B + (image ? r : B + r);
    if (vec_d)
      s2_l1_row<4>(a, b, da, d, g, lane, out);
    else
      s2_l1_row<1>(a, b, da, d, g, lane, out);
  }
}

// The per-row partials in row order (one wave: lane l adds rows l, l + 64, ... in turn, then the fixed DPP tree), each
// sum scaled to this call's share of its term: terms = {sim_ce, scl_logits, scl_image, scl_text}.
__global__ __launch_bounds__(64) void stage2_finish_kernel(const float* __restrict__ work, float* __restrict__ terms,
                                                           int32_t* __restrict__ correct, int B, int C, int d, int n_loc,
                                                           float inv_bg) {
  const int lane = threadIdx.x;
  const int32_t* hits = reinterpret_cast<const int32_t*>(work + 3 * (size_t)B + n_loc);
  float ce = 0.f, kl = 0.f, li = 0.f, lt = 0.f;
  int c = 0;
  for (int r = lane; r < B; r += 64) {
    ce += work[r];
    kl += work[B + r];
    li += work[2 * (size_t)B + r];
    c += hits[r];
  }
  for (int r = lane; r < n_loc; r += 64) lt += work[3 * (size_t)B + r];
  ce = wave_sum(ce);
  kl = wave_sum(kl);
  li = wave_sum(li);
  lt = wave_sum(lt);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if (lane == 0) {
    terms[0] = ce * inv_bg;
    terms[1] = kl * (inv_bg / (float)C);
    terms[2] = li * (inv_bg / (float)d);
    terms[3] = lt / ((float)C * (float)d);
    if (correct) correct[0] = c;
  }
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_vit_fill_special(float* x, const float* class_emb, const float* pos, const float* vpt, int batch,
                                       int tokens, int n_patch, int n_vpt, int width, void* stream) {
  CLIPFS_REQUIRE(x && class_emb && pos && (n_vpt == 0 || vpt), "vit_fill_special: null pointer");
  CLIPFS_REQUIRE(batch > 0 && width > 0 && n_vpt >= 0 && tokens == 1 + n_patch + n_vpt, "vit_fill_special: tokens %d != 1 + %d + %d", tokens, n_patch, n_vpt);
  const size_t total = (size_t)batch * (1 + n_vpt) * width;
  hipLaunchKernelGGL(vit_fill_special_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, class_emb, pos,
                     vpt, batch, tokens, n_patch, n_vpt, width);
  return launch_status();
}

extern "C" int clipfs_text_embed(const int64_t* ids, const float* table, const float* pos, const float* ctx, int n_ctx,
                                 float* x, int n, int seq, int width, void* stream) {
  CLIPFS_REQUIRE(ids && table && pos && x, "text_embed: null pointer");
  CLIPFS_REQUIRE(n > 0 && seq > 0 && width > 0 && (width & 3) == 0 && (!ctx || (n_ctx > 0 && n_ctx < seq)), "text_embed: bad dims");
  CLIPFS_REQUIRE(aligned16(table) && aligned16(pos) && aligned16(x) && (!ctx || aligned16(ctx)), "text_embed: misaligned pointer");
  const size_t total = (size_t)n * seq * (width / 4);
  hipLaunchKernelGGL(text_embed_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, ids, table, pos, ctx,
                     n_ctx, x, n, seq, width);
  return launch_status();
}

extern "C" int clipfs_token_rows_grad(const float* dx, float* dctx, int n, int seq, int width, int n_ctx, int first,
                                      void* stream) {
  CLIPFS_REQUIRE(dx && dctx && n > 0 && n_ctx > 0 && first >= 0 && first + n_ctx <= seq && width > 0, "token_rows_grad: bad args");
  hipLaunchKernelGGL(text_ctx_grad_kernel, dim3((n_ctx * width + 255) / 256), dim3(256), 0, (hipStream_t)stream, dx, dctx,
                     n, seq, width, n_ctx, first);
  return launch_status();
}

extern "C" int clipfs_matmul_small(const float* A, const float* B, float* C, int M, int N, int K, long sam, long sak,
                                   long sbk, long sbn, float alpha, void* stream) {
  CLIPFS_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, "matmul_small: bad args");
  const size_t total = (size_t)M * N;
  hipLaunchKernelGGL(matmul_small_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, B, C,
                     M, N, K, sam, sak, sbk, sbn, alpha);
  return launch_status();
}

extern "C" int clipfs_gather_eot(const float* x, const int64_t* ids, float* out, int32_t* idx_out, int n, int seq,
                                 int width, void* stream) {
  CLIPFS_REQUIRE(x && ids && out && n > 0 && seq > 0 && width > 0, "gather_eot: bad args");
  hipLaunchKernelGGL(gather_eot_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, x, ids, out, idx_out, seq, width);
  return launch_status();
}

extern "C" int clipfs_scatter_rows(const float* dy, const int32_t* idx, float* dx, int n, int seq, int width,
                                   void* stream) {
  CLIPFS_REQUIRE(dy && idx && dx && n > 0 && seq > 0 && width > 0, "scatter_rows: bad args");
  const size_t total = (size_t)n * seq * width;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dy, idx, dx, n, seq,
                     width);
  return launch_status();
}

extern "C" int clipfs_gather_seq_rows(const float* src, size_t ld, const int32_t* idx, float* out, int n, int seq, int width,
                                      void* stream) {
  CLIPFS_REQUIRE(src && idx && out && n > 0 && seq > 0 && width > 0 && ld >= (size_t)width, "gather_seq_rows: bad args");
  hipLaunchKernelGGL(gather_seq_rows_kernel, dim3(grid_for((size_t)n * width)), dim3(256), 0, (hipStream_t)stream, src, ld,
                     idx, out, n, seq, width);
  return launch_status();
}

extern "C" int clipfs_add_seq_rows(const float* src, const int32_t* idx, float* dx, int n, int seq, int width, void* stream) {
  CLIPFS_REQUIRE(src && idx && dx && n > 0 && seq > 0 && width > 0, "add_seq_rows: bad args");
  hipLaunchKernelGGL(add_seq_rows_kernel, dim3(grid_for((size_t)n * width)), dim3(256), 0, (hipStream_t)stream, src, idx, dx,
                     n, seq, width);
  return launch_status();
}

extern "C" int clipfs_put_seq_rows(const float* src, const int32_t* idx, float* dst, size_t ld, int n, int seq, int width,
                                   void* stream) {
  CLIPFS_REQUIRE(src && idx && dst && n > 0 && seq > 0 && width > 0 && ld >= (size_t)width, "put_seq_rows: bad args");
  hipLaunchKernelGGL(put_seq_rows_kernel, dim3(grid_for((size_t)n * width)), dim3(256), 0, (hipStream_t)stream, src, idx, dst,
                     ld, n, seq, width);
  return launch_status();
}

static inline bool rows_map_vec(const void* a, const void* b, size_t ld, int width) {
  return (width % 4) == 0 && (ld % 4) == 0 && aligned16(a) && aligned16(b);
}

extern "C" int clipfs_gather_rows_map(const float* src, size_t ld, const int32_t* map, float* out, int n, int width,
                                      void* stream) {
  CLIPFS_REQUIRE(src && map && out && n > 0 && width > 0 && ld >= (size_t)width, "gather_rows_map: bad args");
  if (rows_map_vec(src, out, ld, width))
    hipLaunchKernelGGL(gather_rows_map_kernel<4>, dim3(grid_for((size_t)n * width / 4)), dim3(256), 0, (hipStream_t)stream,
                       src, ld, map, out, n, width);
  else
    hipLaunchKernelGGL(gather_rows_map_kernel<1>, dim3(grid_for((size_t)n * width)), dim3(256), 0, (hipStream_t)stream, src,
                       ld, map, out, n, width);
  return launch_status();
}

extern "C" int clipfs_put_rows_map(const float* src, const int32_t* map, float* dst, size_t ld, int n, int width,
                                   void* stream) {
  CLIPFS_REQUIRE(src && map && dst && n > 0 && width > 0 && ld >= (size_t)width, "put_rows_map: bad args");
  if (rows_map_vec(src, dst, ld, width))
    hipLaunchKernelGGL(put_rows_map_kernel<4>, dim3(grid_for((size_t)n * width / 4)), dim3(256), 0, (hipStream_t)stream, src,
                       map, dst, ld, n, width);
  else
    hipLaunchKernelGGL(put_rows_map_kernel<1>, dim3(grid_for((size_t)n * width)), dim3(256), 0, (hipStream_t)stream, src, map,
                       dst, ld, n, width);
  return launch_status();
}

extern "C" int clipfs_gather_seq_rows_f16(const void* src_f16, size_t ld, const int32_t* idx, float* out, int n, int seq,
                                          int width, void* stream) {
  CLIPFS_REQUIRE(src_f16 && idx && out && n > 0 && seq > 0 && width > 0 && ld >= (size_t)width, "gather_seq_rows_f16: bad args");
  hipLaunchKernelGGL(gather_seq_rows_f16_kernel, dim3(grid_for((size_t)n * width)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const _Float16*>(src_f16), ld, idx, out, n, seq, width);
  return launch_status();
}

extern "C" int clipfs_put_seq_rows_f16(const float* src, const int32_t* idx, void* dst_f16, size_t ld, int n, int seq,
                                       int width, void* stream) {
  CLIPFS_REQUIRE(src && idx && dst_f16 && n > 0 && seq > 0 && width > 0 && ld >= (size_t)width, "put_seq_rows_f16: bad args");
  hipLaunchKernelGGL(put_seq_rows_f16_kernel, dim3(grid_for((size_t)n * width)), dim3(256), 0, (hipStream_t)stream, src, idx,
                     reinterpret_cast<_Float16*>(dst_f16), ld, n, seq, width);
  return launch_status();
}

extern "C" int clipfs_eot_index(const int64_t* ids, int32_t* idx, int n, int seq, void* stream) {
  CLIPFS_REQUIRE(ids && idx && n > 0 && seq > 0, "eot_index: bad args");
  hipLaunchKernelGGL(eot_index_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, ids, idx, n, seq);
  return launch_status();
}

extern "C" int clipfs_class_mean_fwd(const float* emb, float* out, int classes, int templates, int width, void* stream) {
  CLIPFS_REQUIRE(emb && out && classes > 0 && templates > 0 && width > 0 && width <= 2048, "class_mean_fwd: bad args");
  hipLaunchKernelGGL(class_mean_fwd_kernel, dim3(classes), dim3(64), 0, (hipStream_t)stream, emb, out, templates, width);
  return launch_status();
}

extern "C" int clipfs_class_mean_bwd(const float* emb, const float* dout, float* demb, int classes, int templates,
                                     int width, void* stream) {
  CLIPFS_REQUIRE(emb && dout && demb && classes > 0 && templates > 0 && width > 0 && width <= 2048, "class_mean_bwd: bad args");
  hipLaunchKernelGGL(class_mean_bwd_kernel, dim3(classes), dim3(64), 0, (hipStream_t)stream, emb, dout, demb, templates,
                     width);
  return launch_status();
}

// The two launches of both cross-entropy entry points: the rows kernel, then the fixed-order reduction.  scaler_state
// = NULL for the unscaled gradient.
static int launch_cross_entropy(const float* logits, const int64_t* target, float* dlogits, float* loss_rows,
                                float* loss_sum, int32_t* correct, int rows, int classes, float grad_scale,
                                const float* scaler_state, void* stream) {
  // loss_rows is [2 * rows]: per-row losses, then per-row hit flags (int32) when correct != NULL
  int32_t* flags = correct ? reinterpret_cast<int32_t*>(loss_rows + rows) : nullptr;
  hipLaunchKernelGGL(cross_entropy_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, target,
                     dlogits, loss_rows, flags, rows, classes, grad_scale, scaler_state);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_rows, flags, loss_sum, correct,
                     rows);
  return launch_status();
}

extern "C" int clipfs_cross_entropy(const float* logits, const int64_t* target, float* dlogits, float* loss_rows,
                                    float* loss_sum, int32_t* correct, int rows, int classes, float grad_scale,
                                    void* stream) {
  CLIPFS_REQUIRE(logits && target && loss_rows && loss_sum && rows > 0 && classes > 0, "cross_entropy: bad args");
  return launch_cross_entropy(logits, target, dlogits, loss_rows, loss_sum, correct, rows, classes, grad_scale, nullptr,
                              stream);
}

extern "C" int clipfs_cross_entropy_scaled(const float* logits, const int64_t* target, float* dlogits, float* loss_rows,
                                           float* loss_sum, int32_t* correct, int rows, int classes, float grad_scale,
                                           const float* scaler_state, void* stream) {
  CLIPFS_REQUIRE(logits && target && loss_rows && loss_sum && rows > 0 && classes > 0, "cross_entropy_scaled: bad args");
  CLIPFS_REQUIRE(scaler_state && aligned16(scaler_state), "cross_entropy_scaled: null or misaligned scaler state");
  return launch_cross_entropy(logits, target, dlogits, loss_rows, loss_sum, correct, rows, classes, grad_scale,
                              scaler_state, stream);
}

extern "C" int clipfs_topk(const float* logits, int32_t* labels, int rows, int classes, int k, void* stream) {
  CLIPFS_REQUIRE(logits && labels && rows > 0 && classes > 0 && k > 0 && k <= classes, "topk: bad args");
  hipLaunchKernelGGL(topk_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, logits, labels, classes, k);
  return launch_status();
}

extern "C" int clipfs_channel_affine(const float* x, const float* scale1, const float* bias1, float* y, int rows,
                                     int width, void* stream) {
  CLIPFS_REQUIRE(x && scale1 && bias1 && y && rows > 0 && width > 0, "channel_affine: bad args");
  const size_t total = (size_t)rows * width;
  hipLaunchKernelGGL(channel_affine_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, scale1, bias1, y,
                     total, width);
  return launch_status();
}

extern "C" int clipfs_logit_normalize(const float* z, float* out, float* work, int rows, int classes, void* stream) {
  CLIPFS_REQUIRE(z && out && rows > 0 && classes > 0 && (size_t)rows * classes > 1, "logit_normalize: bad args");
  hipLaunchKernelGGL(logit_normalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, z, out, work, rows, classes);
  return launch_status();
}

extern "C" int clipfs_logit_normalize_bwd(const float* z, const float* dzn, float* dz, int rows, int classes,
                                          void* stream) {
  CLIPFS_REQUIRE(z && dzn && dz && rows > 0 && classes > 0 && (size_t)rows * classes > 1, "logit_normalize_bwd: bad args");
  hipLaunchKernelGGL(logit_normalize_bwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, z, dzn, dz, rows, classes);
  return launch_status();
}

extern "C" int clipfs_colsum(const float* x, const float* y, float* out, int rows, int cols, void* stream) {
  CLIPFS_REQUIRE(x && out && rows > 0 && cols > 0, "colsum: bad args");
  hipLaunchKernelGGL(colsum_kernel, dim3((cols + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y, out, rows, cols);
  return launch_status();
}

// The one AdamW launch behind clipfs_adamw / clipfs_adamw_scaled / clipfs_adamw_ext / clipfs_adamw_tail (each checks
// its own arguments first; the first three pass tail_n = 0).  Without a scaler record the bias corrections come from `step` (>= 1) here; with one the kernel reads them
// from the record and neither `step` nor `grad_scale` is used.
static int launch_adamw(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1,
                        float beta2, float eps, float weight_decay, float grad_scale, const float* scaler_state,
                        const float* clip_state, float* ema_shadow, float ema_decay, void* stream, size_t tail_n = 0,
                        float tail_wd = 0.f, float tail_min = -INFINITY, float tail_max = INFINITY) {
  float inv_sqrt_bc2 = 0.f, step_size = 0.f;  // read from the record when there is one
  if (!scaler_state) {
    const double bc1 = 1.0 - pow((double)beta1, step);
    const double bc2 = 1.0 - pow((double)beta2, step);
    inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    step_size = (float)((double)lr / bc1);
  }
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr,
                     beta1, beta2, eps, weight_decay, inv_sqrt_bc2, step_size, grad_scale, scaler_state, clip_state,
                     ema_shadow, ema_decay, 1.f - ema_decay, n - tail_n, tail_wd, tail_min, tail_max);
  return launch_status();
}

extern "C" int clipfs_adamw(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1,
                            float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
  CLIPFS_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adamw: bad args");
  return launch_adamw(p, g, m, v, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale, nullptr, nullptr, nullptr, 0.f,
                      stream);
}

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

extern "C" int clipfs_grads_nonfinite(const float* g, size_t n, float* scaler_state, void* stream) {
  CLIPFS_REQUIRE(scaler_state && aligned16(scaler_state), "grads_nonfinite: null or misaligned scaler state");
  CLIPFS_REQUIRE(g && aligned4(g), "grads_nonfinite: null or misaligned gradient pointer");
  CLIPFS_REQUIRE(n > 0, "grads_nonfinite: n = 0");
  size_t head = ((16u - (reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) / 4;  // floats before the first 16-byte boundary
  if (head > n) head = n;
  hipLaunchKernelGGL(grads_nonfinite_kernel, dim3(grid_for((n - head) / 4)), dim3(256), 0, (hipStream_t)stream, g, n,
                     (unsigned)head, reinterpret_cast<int32_t*>(scaler_state));
  return launch_status();
}

extern "C" int clipfs_scaler_decide(float* scaler_state, float lr, float beta1, float beta2, float growth_factor,
                                    float backoff_factor, int growth_interval, void* stream) {
  CLIPFS_REQUIRE(scaler_state && aligned16(scaler_state), "scaler_decide: null or misaligned scaler state");
  CLIPFS_REQUIRE(growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f && growth_interval >= 0,
                 "scaler_decide: growth_factor %g must be >= 1, backoff_factor %g in (0, 1], growth_interval %d >= 0",
                 (double)growth_factor, (double)backoff_factor, growth_interval);
  hipLaunchKernelGGL(scaler_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scaler_state, lr, beta1, beta2,
                     growth_factor, backoff_factor, growth_interval);
  return launch_status();
}

extern "C" int clipfs_adamw_scaled(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, const float* scaler_state, void* stream) {
  CLIPFS_REQUIRE(scaler_state && aligned16(scaler_state), "adamw_scaled: null or misaligned scaler state");
  CLIPFS_REQUIRE(p && g && m && v && aligned4(p) && aligned4(g) && aligned4(m) && aligned4(v),
                 "adamw_scaled: null or misaligned pointer");
  CLIPFS_REQUIRE(n > 0, "adamw_scaled: n = 0");
  return launch_adamw(p, g, m, v, n, 0, lr, beta1, beta2, eps, weight_decay, 1.f, scaler_state, nullptr, nullptr, 0.f,
                      stream);
}

extern "C" size_t clipfs_grad_sumsq_work_doubles(size_t n) { return sumsq_chunks(n); }

extern "C" int clipfs_grad_sumsq(const float* g, size_t n, double* work, void* stream) {
  CLIPFS_REQUIRE(g && aligned4(g), "grad_sumsq: null or misaligned gradient pointer");
  CLIPFS_REQUIRE(work && (reinterpret_cast<uintptr_t>(work) & 7u) == 0, "grad_sumsq: null or misaligned work buffer");
  CLIPFS_REQUIRE(n > 0, "grad_sumsq: n = 0");
  const unsigned head = (unsigned)(((16u - (reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) / 4);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)sumsq_chunks(n)), dim3(256), 0, (hipStream_t)stream, g, n,
                     sumsq_chunk_elems(n), head, work);
  return launch_status();
}

extern "C" int clipfs_clip_decide(const double* work, size_t n, float max_norm, const float* scaler_state,
                                  float* clip_state, void* stream) {
  CLIPFS_REQUIRE(clip_state && aligned16(clip_state), "clip_decide: null or misaligned clip state");
  CLIPFS_REQUIRE(!scaler_state || aligned16(scaler_state), "clip_decide: misaligned scaler state");
  CLIPFS_REQUIRE(work && (reinterpret_cast<uintptr_t>(work) & 7u) == 0, "clip_decide: null or misaligned work buffer");
  CLIPFS_REQUIRE(n > 0, "clip_decide: n = 0");
  CLIPFS_REQUIRE(max_norm > 0.f && max_norm <= 3.402823466e38f, "clip_decide: max_norm %g must be positive and finite",
                 (double)max_norm);
  hipLaunchKernelGGL(clip_decide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, work, (int)sumsq_chunks(n), max_norm,
                     scaler_state, clip_state);
  return launch_status();
}

extern "C" int clipfs_adamw_ext(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1,
                                float beta2, float eps, float weight_decay, float grad_scale, const float* scaler_state,
                                const float* clip_state, float* ema_shadow, float ema_decay, void* stream) {
  CLIPFS_REQUIRE(p && g && m && v && aligned4(p) && aligned4(g) && aligned4(m) && aligned4(v),
                 "adamw_ext: null or misaligned pointer");
  CLIPFS_REQUIRE(!scaler_state || aligned16(scaler_state), "adamw_ext: misaligned scaler state");
  CLIPFS_REQUIRE(!clip_state || aligned16(clip_state), "adamw_ext: misaligned clip state");
  CLIPFS_REQUIRE(!ema_shadow || (aligned4(ema_shadow) && ema_shadow != p && ema_shadow != m && ema_shadow != v),
                 "adamw_ext: misaligned or aliased ema shadow");
  CLIPFS_REQUIRE(!ema_shadow || (ema_decay > 0.f && ema_decay < 1.f), "adamw_ext: ema_decay %g must lie in (0, 1)",
                 (double)ema_decay);
  CLIPFS_REQUIRE(n > 0, "adamw_ext: n = 0");
  CLIPFS_REQUIRE(scaler_state || step >= 1, "adamw_ext: step %d must be >= 1 without a scaler state", step);
  return launch_adamw(p, g, m, v, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale, scaler_state, clip_state,
                      ema_shadow, ema_decay, stream);
}

extern "C" int clipfs_adamw_tail(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, float grad_scale, const float* scaler_state,
                                 const float* clip_state, float* ema_shadow, float ema_decay, size_t tail_n,
                                 float tail_weight_decay, float tail_min, float tail_max, void* stream) {
  CLIPFS_REQUIRE(p && g && m && v && aligned4(p) && aligned4(g) && aligned4(m) && aligned4(v),
                 "adamw_tail: null or misaligned pointer");
  CLIPFS_REQUIRE(!scaler_state || aligned16(scaler_state), "adamw_tail: misaligned scaler state");
  CLIPFS_REQUIRE(!clip_state || aligned16(clip_state), "adamw_tail: misaligned clip state");
  CLIPFS_REQUIRE(!ema_shadow || (aligned4(ema_shadow) && ema_shadow != p && ema_shadow != m && ema_shadow != v),
                 "adamw_tail: misaligned or aliased ema shadow");
  CLIPFS_REQUIRE(!ema_shadow || (ema_decay > 0.f && ema_decay < 1.f), "adamw_tail: ema_decay %g must lie in (0, 1)",
                 (double)ema_decay);
  CLIPFS_REQUIRE(n > 0, "adamw_tail: n = 0");
  CLIPFS_REQUIRE(scaler_state || step >= 1, "adamw_tail: step %d must be >= 1 without a scaler state", step);
  CLIPFS_REQUIRE(tail_n <= n, "adamw_tail: tail_n = %zu exceeds n = %zu", tail_n, n);
  CLIPFS_REQUIRE(tail_min == tail_min && tail_max == tail_max, "adamw_tail: tail_min or tail_max is NaN");
  CLIPFS_REQUIRE(tail_min <= tail_max, "adamw_tail: tail_min = %g exceeds tail_max = %g", (double)tail_min, (double)tail_max);
  return launch_adamw(p, g, m, v, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale, scaler_state, clip_state,
                      ema_shadow, ema_decay, stream, tail_n, tail_weight_decay, tail_min, tail_max);
}

extern "C" int clipfs_l1_loss(const float* a, const float* b, size_t n, float* loss, float* da, float grad_scale,
                              void* stream) {
  CLIPFS_REQUIRE(a && b && loss && n > 0, "l1_loss: bad args");
  hipLaunchKernelGGL(l1_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, b, n, loss, da, grad_scale);
  return launch_status();
}

extern "C" int clipfs_kl_logits(const float* logits, const float* target_logits, float* loss_rows, float* dlogits,
                                int rows, int classes, float grad_scale, void* stream) {
  CLIPFS_REQUIRE(logits && target_logits && loss_rows && rows > 0 && classes > 0, "kl_logits: bad args");
  hipLaunchKernelGGL(kl_logits_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, target_logits,
                     loss_rows, dlogits, rows, classes, grad_scale);
  return launch_status();
}

extern "C" int clipfs_stage2_objective(const float* cos, const float* zs_logits, const int64_t* target, const float* img,
                                       const float* zs_img, const float* txt, const float* zs_txt, float* dcos,
                                       float* dimg, float* dtxt, float* work, float* terms, int32_t* correct, int B,
                                       int C, int d, int C_loc, float inv_global_batch, const float* scaler_state,
                                       void* stream) {
  CLIPFS_REQUIRE(B > 0 && C > 0 && d > 0, "stage2_objective: sizes B %d, C %d, d %d must be positive", B, C, d);
  CLIPFS_REQUIRE(C_loc >= 0 && C_loc <= C, "stage2_objective: C_loc %d outside [0, C = %d]", C_loc, C);
  CLIPFS_REQUIRE(2 * (long long)B + C_loc <= 0x7ffffff0LL, "stage2_objective: 2 B + C_loc = %lld rows is too many",
                 2 * (long long)B + C_loc);
  CLIPFS_REQUIRE(cos && zs_logits && target, "stage2_objective: null pointer (cos, zs_logits or target)");
  CLIPFS_REQUIRE(img && zs_img, "stage2_objective: null pointer (img or zs_img)");
  CLIPFS_REQUIRE(C_loc == 0 || (txt && zs_txt), "stage2_objective: null pointer (txt or zs_txt with C_loc %d)", C_loc);
  CLIPFS_REQUIRE(work && terms, "stage2_objective: null pointer (work or terms)");
  CLIPFS_REQUIRE(aligned4(cos) && aligned4(zs_logits) && aligned4(img) && aligned4(zs_img) && aligned4(txt) &&
                     aligned4(zs_txt) && aligned4(dcos) && aligned4(dimg) && aligned4(dtxt) && aligned4(work) &&
                     aligned4(terms) && aligned4(correct) && (reinterpret_cast<uintptr_t>(target) & 7u) == 0,
                 "stage2_objective: misaligned pointer");
  CLIPFS_REQUIRE(!scaler_state || aligned16(scaler_state), "stage2_objective: misaligned scaler state");
  CLIPFS_REQUIRE(inv_global_batch > 0.f && inv_global_batch <= 3.402823466e38f,
                 "stage2_objective: inv_global_batch %g must be positive and finite", (double)inv_global_batch);
  const bool txt16 = C_loc == 0 || (aligned16(txt) && aligned16(zs_txt) && aligned16(dtxt));
  const int vec_c = (C % 4 == 0 && aligned16(cos) && aligned16(zs_logits) && aligned16(dcos)) ? 1 : 0;
  const int vec_d = (d % 4 == 0 && aligned16(img) && aligned16(zs_img) && aligned16(dimg) && txt16) ? 1 : 0;
  const unsigned rows = 2u * (unsigned)B + (unsigned)C_loc;
  hipLaunchKernelGGL(stage2_objective_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, cos, zs_logits,
                     target, img, zs_img, txt, zs_txt, dcos, dimg, dtxt, work, B, C, d, C_loc, inv_global_batch,
                     scaler_state, vec_c, vec_d);
  CLIPFS_CHECK(launch_status());
  hipLaunchKernelGGL(stage2_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, work, terms, correct, B, C, d, C_loc,
                     inv_global_batch);
  return launch_status();
}
