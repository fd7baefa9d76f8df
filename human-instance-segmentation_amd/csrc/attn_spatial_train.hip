// SpatialAttentionModule (attention_modules.py:67-113) in training (gfx950): forward (+ Dropout2d) and backward.
// HBM-streaming kernels; the 7x7 weight gradient goes through per-row partials and sum_rows (no atomics).  The
// attention map itself is misc.hip's attn_map_kernel, the inference forward's.
#include <float.h>
#include "train_norm.h"
#include "hiseg_head_train.h"

namespace hiseg {

static inline unsigned nb(long long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// stats[p] = (mean_c x, max_c x), argmax[p] = first channel attaining the max.
template <typename T>
__global__ void __launch_bounds__(256) sa_stats_kernel(const void* x, long long P, int C, float* stats, int* argmax) {
  constexpr int K = Chunk<T>::N;
  constexpr int G = 16;
  const int nch = C / K;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix = gid / G;
  const int l = (int)(gid % G);
  float s = 0.f, m = -FLT_MAX, v[K];
  int am = 0x7fffffff;
  if (pix < P) {
    const uint4* src = reinterpret_cast<const uint4*>(x) + pix * nch;
    for (int ch = l; ch < nch; ch += G) {
      Chunk<T>::unpack(src[ch], v);
#pragma unroll
      for (int e = 0; e < K; ++e) {
        s += v[e];
        if (v[e] > m) { m = v[e]; am = ch * K + e; }
      }
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, G);
    const float mo = __shfl_xor(m, off, G);
    const int ao = __shfl_xor(am, off, G);
    if (mo > m || (mo == m && ao < am)) { m = mo; am = ao; }
  }
  if (pix < P && l == 0) {
    stats[pix * 2] = s / (float)C;
    stats[pix * 2 + 1] = m;
    argmax[pix] = am;
  }
}

// out = x * att[p] * mul[n][c]
template <typename T>
__global__ void __launch_bounds__(256) sa_apply_kernel(const void* x, long long P, int HW, int C, const float* att,
                                                       const float* mul, void* out) {
  constexpr int K = Chunk<T>::N;
  const int nch = C / K;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= P * nch) return;
  const long long p = gid / nch;
  const int ch = (int)(gid - p * nch);
  const float a = att[p];
  float v[K];
  Chunk<T>::unpack(reinterpret_cast<const uint4*>(x)[gid], v);
  const float* m = mul ? mul + (p / HW) * C + ch * K : nullptr;
#pragma unroll
  for (int e = 0; e < K; ++e) v[e] *= m ? a * m[e] : a;
  reinterpret_cast<uint4*>(out)[gid] = Chunk<T>::pack(v);
}

// dpre[p] = (sum_c dout*mul*x) * att * (1 - att)
template <typename T>
__global__ void __launch_bounds__(256) sa_bwd1_kernel(const void* x, const void* dout, long long P, int HW, int C,
                                                      const float* att, const float* mul, float* dpre) {
  constexpr int K = Chunk<T>::N;
  constexpr int G = 16;
  const int nch = C / K;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix = gid / G;
  const int l = (int)(gid % G);
  float s = 0.f, v[K], g[K];
  if (pix < P) {
    const uint4* xs = reinterpret_cast<const uint4*>(x) + pix * nch;
    const uint4* ds = reinterpret_cast<const uint4*>(dout) + pix * nch;
    const float* m = mul ? mul + (pix / HW) * C : nullptr;
    for (int ch = l; ch < nch; ch += G) {
      Chunk<T>::unpack(xs[ch], v);
      Chunk<T>::unpack(ds[ch], g);
#pragma unroll
      for (int e = 0; e < K; ++e) s += g[e] * v[e] * (m ? m[ch * K + e] : 1.f);
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, G);
  if (pix < P && l == 0) {
    const float a = att[pix];
    dpre[pix] = s * a * (1.f - a);
  }
}

// dstats[p][c] = sum_taps w[c][ky][kx] * dpre[y - ky + r][x - kx + r]   (adjoint of the 7x7 correlation)
__global__ void __launch_bounds__(256) sa_bwd2_kernel(const float* dpre, int N, int H, int W, const float* w, int k,
                                                      float* dstats) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)N * H * W) return;
  const int x = (int)(gid % W);
  const long long t = gid / W;
  const int y = (int)(t % H);
  const int n = (int)(t / H);
  const int r = k / 2;
  float a0 = 0.f, a1 = 0.f;
  for (int ky = 0; ky < k; ++ky) {
    const int yy = y - ky + r;
    if (yy < 0 || yy >= H) continue;
    for (int kx = 0; kx < k; ++kx) {
      const int xx = x - kx + r;
      if (xx < 0 || xx >= W) continue;
      const float d = dpre[((long long)n * H + yy) * W + xx];
      a0 += w[ky * k + kx] * d;
      a1 += w[(k + ky) * k + kx] * d;
    }
  }
  dstats[gid * 2] = a0;
  dstats[gid * 2 + 1] = a1;
}

// dw partial per image row: part[(n*H + y)][c*k*k + ky*k + kx] = sum_x dpre[y][x] * stats[y+ky-r][x+kx-r][c]
__global__ void __launch_bounds__(256) sa_dw_kernel(const float* dpre, const float* stats, int N, int H, int W, int k,
                                                    float* part) {
  const int row = blockIdx.x;  // n*H + y
  const int n = row / H, y = row - n * H;
  const int t = threadIdx.x;
  const int nw = 2 * k * k;
  if (t >= nw) return;
  const int c = t / (k * k), ky = (t / k) % k, kx = t % k;
  const int r = k / 2;
  const int yy = y + ky - r;
  float acc = 0.f;
  if (yy >= 0 && yy < H) {
    for (int x = 0; x < W; ++x) {
      const int xx = x + kx - r;
      if (xx < 0 || xx >= W) continue;
      acc += dpre[((long long)n * H + y) * W + x] * stats[(((long long)n * H + yy) * W + xx) * 2 + c];
    }
  }
  part[(long long)row * nw + t] = acc;
}

// dx = dout*mul*att + dstats0 / C + [c == argmax] * dstats1
template <typename T>
__global__ void __launch_bounds__(256) sa_bwd3_kernel(const void* dout, long long P, int HW, int C, const float* att,
                                                      const float* mul, const float* dstats, const int* argmax, void* dx) {
  constexpr int K = Chunk<T>::N;
  const int nch = C / K;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= P * nch) return;
  const long long p = gid / nch;
  const int ch = (int)(gid - p * nch);
  const float a = att[p], d0 = dstats[p * 2] / (float)C, d1 = dstats[p * 2 + 1];
  const int am = argmax[p];
  const float* m = mul ? mul + (p / HW) * C + ch * K : nullptr;
  float g[K];
  Chunk<T>::unpack(reinterpret_cast<const uint4*>(dout)[gid], g);
#pragma unroll
  for (int e = 0; e < K; ++e) {
    float v = g[e] * a * (m ? m[e] : 1.f) + d0;
    if (ch * K + e == am) v += d1;
    g[e] = v;
  }
  reinterpret_cast<uint4*>(dx)[gid] = Chunk<T>::pack(g);
}

}  // namespace hiseg

using namespace hiseg;

extern "C" int hiseg_attn_spatial_train_fwd(int dtype, const void* x, int N, int H, int W, int C, const float* w7, int k,
                                            const float* chan_mul, float* stats, int* argmax, float* att, void* out,
                                            hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w7 && stats && argmax && att && out && N > 0 && H > 0 && W > 0 && (k & 1), HISEG_ERR_BAD_ARG,
                "attn_spatial_train_fwd: bad args");
  HISEG_REQUIRE(C > 0 && C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "attn_spatial_train_fwd: C alignment");
  hipStream_t s = (hipStream_t)stream;
  const long long P = (long long)N * H * W;
  DISPATCH_T(dtype, hipLaunchKernelGGL(sa_stats_kernel<T>, dim3(nb(P * 16, 256)), dim3(256), 0, s, x, P, C, stats, argmax));
  attn_map_launch(stats, N, H, W, w7, k, att, s);
  DISPATCH_T(dtype, hipLaunchKernelGGL(sa_apply_kernel<T>, dim3(nb(P * (C / chunk_of(dtype)), 256)), dim3(256), 0, s, x,
                                       P, H * W, C, att, chan_mul, out));
  return hiseg_check_launch("attn_spatial_train_fwd");
}

extern "C" int hiseg_attn_spatial_ws(int N, int H, int W, int k) {
  // floats: dpre [P] + dstats [2P] + dw partial [N*H][2k^2]
  const long long P = (long long)N * H * W;
  return (int)(3 * P + (long long)N * H * 2 * k * k);
}

extern "C" int hiseg_attn_spatial_bwd(int dtype, const void* x, int N, int H, int W, int C, const float* w7, int k,
                                      const float* chan_mul, const float* stats, const int* argmax, const float* att,
                                      const void* dout, void* dx, float* ws, float* dw7, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w7 && stats && argmax && att && dout && dx && ws && dw7, HISEG_ERR_BAD_ARG, "attn_spatial_bwd: null");
  HISEG_REQUIRE(C > 0 && C % chunk_of(dtype) == 0 && (k & 1) && 2 * k * k <= 256, HISEG_ERR_BAD_SHAPE,
                "attn_spatial_bwd: shape");
  hipStream_t s = (hipStream_t)stream;
  const long long P = (long long)N * H * W;
  float* dpre = ws;
  float* dstats = ws + P;
  float* part = ws + 3 * P;
  DISPATCH_T(dtype, hipLaunchKernelGGL(sa_bwd1_kernel<T>, dim3(nb(P * 16, 256)), dim3(256), 0, s, x, dout, P, H * W, C,
                                       att, chan_mul, dpre));
  hipLaunchKernelGGL(sa_bwd2_kernel, dim3(nb(P, 256)), dim3(256), 0, s, dpre, N, H, W, w7, k, dstats);
  hipLaunchKernelGGL(sa_dw_kernel, dim3(N * H), dim3(256), 0, s, dpre, stats, N, H, W, k, part);
  sum_rows(part, N * H, 2 * k * k, 2 * k * k, dw7, 1, s);
  DISPATCH_T(dtype, hipLaunchKernelGGL(sa_bwd3_kernel<T>, dim3(nb(P * (C / chunk_of(dtype)), 256)), dim3(256), 0, s,
                                       dout, P, H * W, C, att, chan_mul, dstats, argmax, dx));
  return hiseg_check_launch("attn_spatial_bwd");
}
