// Data-movement kernels of the MoCo-v3 ResNet-50 auxiliary branch (slow_pace.py:1237-1271 load_moco,
// :1677-1680 loss_aux; the model itself is jittor.models.resnet.resnet50 = torchvision's ResNet-50 v1.5).
// The branch is a FROZEN feature extractor run forward only.  Every convolution is a GEMM on the fp32-MFMA kernel
// (gemm.hip): activations are NHWC, so a 1x1 / stride-1 convolution IS a GEMM on the activation tensor, and the
// others read an im2col matrix written by the kernel below; BatchNorm (inference statistics) is folded into the
// convolution's weights and bias on the host, ReLU (after the residual add) is the GEMM epilogue's act 3.
// What is left for this file: the NCHW -> NHWC input permute, im2col, the 3x3/2 max pool and the global average pool
// -- all HBM-bound gathers with 16-byte accesses along the channel axis.  CLIP's ModifiedResNet (clipfs/resnet.py:
// ClipResNet) runs on the same kernels plus a k x k mean pool and the two kernels of its attention-pool head.
#include "common.h"

namespace clipfs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// x [N, C, H, W] -> y [N, H, W, C]
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int C,
                                                            int H, int W) {
  const size_t total = (size_t)N * H * W * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    size_t p = i / C;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H);
    const int n = (int)(p / H);
    y[i] = x[(((size_t)n * C + c) * H + h) * W + w];
  }
}

// x [N, H, W, C] -> col [N * Ho * Wo, Kp], column (ky, kx, c) (c fastest), columns [kh*kw*C, Kp) zero.
// CV = channels moved per thread (4 when C % 4 == 0: 16-byte loads / stores, else 1)
template <int CV>
__global__ __launch_bounds__(256) void im2col_nhwc_kernel(const float* __restrict__ x, float* __restrict__ col, int N, int H,
                                                           int W, int C, int kh, int kw, int stride, int pad, int Ho, int Wo,
                                                           int Kp) {
  const int kcols = Kp / CV;
  const size_t total = (size_t)N * Ho * Wo * kcols;
  const int K = kh * kw * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int kc = (int)(i % kcols) * CV;
    size_t m = i / kcols;
    const int wo = (int)(m % Wo);
    size_t q = m / Wo;
    const int ho = (int)(q % Ho);
    const int n = (int)(q / Ho);
    float v[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) v[e] = 0.f;
    if (kc < K) {
      const int c = kc % C, t = kc / C;
      const int kx = t % kw, ky = t / kw;
      const int hi = ho * stride - pad + ky, wi = wo * stride - pad + kx;
      if (hi >= 0 && hi < H && wi >= 0 && wi < W) {
        const float* src = x + (((size_t)n * H + hi) * W + wi) * C + c;
        if (CV == 4) {
          const f32x4 u = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
          for (int e = 0; e < CV; ++e) v[e] = u[e];
        } else {
          v[0] = src[0];
        }
      }
    }
    float* dst = col + m * Kp + kc;
    if (CV == 4)
      *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1 % CV], v[2 % CV], v[3 % CV]};
    else
      dst[0] = v[0];
  }
}

// 3x3 / stride 2 / pad 1 max pool on NHWC (C % 4 == 0); padding never wins (-inf)
__global__ __launch_bounds__(256) void maxpool3x3s2_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H,
                                                                 int W, int C, int Ho, int Wo) {
  const int c4n = C / 4;
  const size_t total = (size_t)N * Ho * Wo * c4n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c4n) * 4;
    size_t m = i / c4n;
    const int wo = (int)(m % Wo);
    size_t q = m / Wo;
    const int ho = (int)(q % Ho);
    const int n = (int)(q / Ho);
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int hi = 2 * ho - 1 + ky, wi = 2 * wo - 1 + kx;
        if (hi >= 0 && hi < H && wi >= 0 && wi < W) {
          const f32x4 u = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + hi) * W + wi) * C + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) best[e] = fmaxf(best[e], u[e]);
        }
      }
    *reinterpret_cast<f32x4*>(y + m * C + c) = best;
  }
}

// y[n, c] = mean over the HW positions of x[n, :, c]   (one wave per (n, 64-channel group): lanes = channels)
__global__ __launch_bounds__(64) void global_avgpool_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int HW,
                                                                 int C) {
  const int groups = (C + 63) / 64;
  const int n = blockIdx.x / groups, c = (blockIdx.x % groups) * 64 + threadIdx.x;
  if (c >= C) return;
  const float* p = x + (size_t)n * HW * C + c;
  float s = 0.f;
  for (int i = 0; i < HW; ++i) s += p[(size_t)i * C];  // sequential over positions: the summation order of a plain loop
  y[(size_t)n * C + c] = s / (float)HW;
}

// ---- CLIP's ModifiedResNet (jclip/model_res.py:84-170 = the published CLIP ModifiedResNet): the same GEMM convolutions,
// plus the three kernels below -- k x k mean pools instead of strided convolutions, and the attention-pool head.

// k x k mean, stride k, no padding, output floor(H/k) x floor(W/k) (rows / columns past the last full window are never
// read).  Sum order: row-major inside the window.
__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H,
                                                            int W, int C, int k, int Ho, int Wo) {
  const int c4n = C / 4;
  const size_t total = (size_t)N * Ho * Wo * c4n;
  const float inv = 1.f / (float)(k * k);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c4n) * 4;
    size_t m = i / c4n;
    const int wo = (int)(m % Wo);
    size_t q = m / Wo;
    const int ho = (int)(q % Ho);
    const int n = (int)(q / Ho);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < k; ++ky) {
      const float* row = x + (((size_t)n * H + (size_t)ho * k + ky) * W + (size_t)wo * k) * C + c;
      for (int kx = 0; kx < k; ++kx) s += *reinterpret_cast<const f32x4*>(row + (size_t)kx * C);
    }
    *reinterpret_cast<f32x4*>(y + m * C + c) = s * inv;
  }
}

// tok[n, 0, :] = mean_i x[n, i, :] + pos[0];  tok[n, 1 + i, :] = x[n, i, :] + pos[1 + i]   (x [N, HW, C], tok [N, HW+1, C]).
// One thread per (image, 4 channels) walks the HW rows once: the row is copied and added to the running sum (i ascending).
__global__ __launch_bounds__(256) void attnpool_tokens_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                               float* __restrict__ tok, int N, int HW, int C) {
  const int c4n = C / 4;
  const size_t total = (size_t)N * c4n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c4n) * 4;
    const size_t n = i / c4n;
    const float* xs = x + n * HW * C + c;
    float* ts = tok + n * (HW + 1) * C + c;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < HW; ++r) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(xs + (size_t)r * C);
      s += u;
      *reinterpret_cast<f32x4*>(ts + (size_t)(r + 1) * C) = u + *reinterpret_cast<const f32x4*>(pos + (size_t)(r + 1) * C + c);
    }
    *reinterpret_cast<f32x4*>(ts) = s / (float)HW + *reinterpret_cast<const f32x4*>(pos + c);
  }
}

// out[n, h*64 ...] = softmax_j(q[n, h] . k[n, j, h] / 8) . v[n, j, h]: the attention pool reads query row 0 only.
// One wave per (image, head).  A key / value row of the head is 64 floats = 16 lanes x 16 bytes, so the wave takes four rows
// per step (lane group g = lane / 16 takes rows g, g + 4, ...); the scores go through LDS, max and sum are wave reductions,
// every summation order is fixed.
constexpr int ATTNPOOL_MAX_L = 1024;
constexpr int ATTNPOOL_MAX_HEADS = 128;

__global__ __launch_bounds__(64) void attnpool_attend_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                              float* __restrict__ out, int L, int heads) {
  __shared__ float sc[ATTNPOOL_MAX_L];
  const int n = blockIdx.x / heads, h = blockIdx.x % heads;
  const int lane = threadIdx.x, grp = lane >> 4, sub = (lane & 15) * 4;
  const int width = heads * 64;
  const size_t ldkv = (size_t)2 * width;
  const float* kbase = kv + (size_t)n * L * ldkv + (size_t)h * 64 + sub;
  const float* vbase = kbase + width;
  const f32x4 qv = *reinterpret_cast<const f32x4*>(q + (size_t)n * width + (size_t)h * 64 + sub);
  for (int j0 = 0; j0 < L; j0 += 4) {
    const int j = j0 + grp;
    float d = 0.f;
    if (j < L) {
      const f32x4 kk = *reinterpret_cast<const f32x4*>(kbase + (size_t)j * ldkv);
      d = qv[0] * kk[0] + qv[1] * kk[1] + qv[2] * kk[2] + qv[3] * kk[3];
    }
    d += __shfl_xor(d, 1);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 4);
    d += __shfl_xor(d, 8);
    if (j < L && (lane & 15) == 0) sc[j] = d * 0.125f;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int j = lane; j < L; j += 64) mx = fmaxf(mx, sc[j]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < L; j += 64) {
    const float p = expf(sc[j] - mx);
    sc[j] = p;
    sum += p;
  }
  sum = wave_sum(sum);
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = grp; j < L; j += 4) acc += sc[j] * *reinterpret_cast<const f32x4*>(vbase + (size_t)j * ldkv);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    acc[e] += __shfl_xor(acc[e], 16);
    acc[e] += __shfl_xor(acc[e], 32);
  }
  if (grp == 0) *reinterpret_cast<f32x4*>(out + (size_t)n * width + (size_t)h * 64 + sub) = acc / sum;
}

static inline unsigned rn_grid(size_t total) {
  const size_t b = (total + 255) / 256;
  return (unsigned)(b > 65535 ? 65535 : (b < 1 ? 1 : b));
}

}  // namespace clipfs

using namespace clipfs;

extern "C" int clipfs_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, void* stream) {
  CLIPFS_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0, "nchw_to_nhwc: bad args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(rn_grid((size_t)N * C * H * W)), dim3(256), 0, (hipStream_t)stream, x, y, N, C, H,
                     W);
  return launch_status();
}

extern "C" int clipfs_im2col_nhwc(const float* x, float* col, int N, int H, int W, int C, int kh, int kw, int stride, int pad,
                                  int Kp, void* stream) {
  CLIPFS_REQUIRE(x && col && N > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0,
                 "im2col_nhwc: bad args");
  CLIPFS_REQUIRE(Kp >= kh * kw * C && (Kp & 3) == 0, "im2col_nhwc: Kp %d must be >= kh*kw*C and a multiple of 4", Kp);
  const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
  CLIPFS_REQUIRE(Ho > 0 && Wo > 0, "im2col_nhwc: empty output");
  hipStream_t st = (hipStream_t)stream;
  if ((C & 3) == 0 && aligned16(x) && aligned16(col)) {
    const size_t total = (size_t)N * Ho * Wo * (Kp / 4);
    hipLaunchKernelGGL((im2col_nhwc_kernel<4>), dim3(rn_grid(total)), dim3(256), 0, st, x, col, N, H, W, C, kh, kw, stride, pad,
                       Ho, Wo, Kp);
  } else {
    const size_t total = (size_t)N * Ho * Wo * Kp;
    hipLaunchKernelGGL((im2col_nhwc_kernel<1>), dim3(rn_grid(total)), dim3(256), 0, st, x, col, N, H, W, C, kh, kw, stride, pad,
                       Ho, Wo, Kp);
  }
  return launch_status();
}

extern "C" int clipfs_maxpool3x3s2_nhwc(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  CLIPFS_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && aligned16(x) && aligned16(y),
                 "maxpool3x3s2_nhwc: bad args (C %% 4 == 0, 16-byte aligned)");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  hipLaunchKernelGGL(maxpool3x3s2_nhwc_kernel, dim3(rn_grid((size_t)N * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                     x, y, N, H, W, C, Ho, Wo);
  return launch_status();
}

extern "C" int clipfs_global_avgpool_nhwc(const float* x, float* y, int N, int HW, int C, void* stream) {
  CLIPFS_REQUIRE(x && y && N > 0 && HW > 0 && C > 0, "global_avgpool_nhwc: bad args");
  hipLaunchKernelGGL(global_avgpool_nhwc_kernel, dim3(N * ((C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, x, y, HW, C);
  return launch_status();
}

extern "C" int clipfs_avgpool_nhwc(const float* x, float* y, int N, int H, int W, int C, int k, void* stream) {
  CLIPFS_REQUIRE(x && y && aligned16(x) && aligned16(y), "avgpool_nhwc: x and y must be non-null and 16-byte aligned");
  CLIPFS_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0, "avgpool_nhwc: bad shape (C %d must be a multiple of 4)", C);
  CLIPFS_REQUIRE(k >= 1 && k <= H && k <= W, "avgpool_nhwc: window k %d outside [1, min(H, W)]", k);
  const int Ho = H / k, Wo = W / k;
  hipLaunchKernelGGL(avgpool_nhwc_kernel, dim3(rn_grid((size_t)N * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, y,
                     N, H, W, C, k, Ho, Wo);
  return launch_status();
}

extern "C" int clipfs_attnpool_tokens(const float* x, const float* pos, float* tok, int N, int HW, int C, void* stream) {
  CLIPFS_REQUIRE(x && pos && tok && aligned16(x) && aligned16(pos) && aligned16(tok),
                 "attnpool_tokens: x, pos and tok must be non-null and 16-byte aligned");
  CLIPFS_REQUIRE(N > 0 && HW > 0 && C > 0 && (C & 3) == 0, "attnpool_tokens: bad shape (C %d must be a multiple of 4)", C);
  hipLaunchKernelGGL(attnpool_tokens_kernel, dim3(rn_grid((size_t)N * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, pos, tok,
                     N, HW, C);
  return launch_status();
}

extern "C" int clipfs_attnpool_attend(const float* q, const float* kv, float* out, int N, int L, int heads, void* stream) {
  CLIPFS_REQUIRE(q && kv && out && aligned16(q) && aligned16(kv) && aligned16(out),
                 "attnpool_attend: q, kv and out must be non-null and 16-byte aligned");
  CLIPFS_REQUIRE(L >= 2 && L <= ATTNPOOL_MAX_L, "attnpool_attend: L %d outside [2, %d]", L, ATTNPOOL_MAX_L);
  CLIPFS_REQUIRE(heads >= 1 && heads <= ATTNPOOL_MAX_HEADS, "attnpool_attend: heads %d outside [1, %d]", heads,
                 ATTNPOOL_MAX_HEADS);
  CLIPFS_REQUIRE(N > 0 && (long long)N * heads <= 0x7fffffffLL, "attnpool_attend: bad batch %d", N);
  hipLaunchKernelGGL(attnpool_attend_kernel, dim3((unsigned)(N * heads)), dim3(64), 0, (hipStream_t)stream, q, kv, out, L,
                     heads);
  return launch_status();
}
