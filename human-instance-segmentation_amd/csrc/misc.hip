// Memory-bound kernels of the hot path (pool, spatial attention, input prologue, layout and epilogue
// kernels; the depthwise convs are in dwconv.hip, the SqueezeExcite gate in se_gate.hip).  All are vectorised on
// 16-B chunks of the NHWC channel dimension (cdna_hip_programming.md Guideline 13) and grid-sized for 256 CUs.
#include <float.h>
#include "common.h"
#include "head2.h"

namespace hiseg {

// ------------------------------------------------------------------ MaxPool2d(2), NHWC
template <typename T>
__global__ void __launch_bounds__(256) maxpool2x2_kernel(const void* in, int N, int H, int W, int C, void* out) {
  constexpr int K = Chunk<T>::N;
  const int nch = C / K;
  const int Ho = H / 2, Wo = W / 2;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)N * Ho * Wo * nch;
  if (gid >= total) return;
  const int ch = (int)(gid % nch);
  long long p = gid / nch;
  const int x = (int)(p % Wo); p /= Wo;
  const int y = (int)(p % Ho);
  const int n = (int)(p / Ho);
  const uint4* src = reinterpret_cast<const uint4*>(in);
  float m[K], v[K];
  for (int e = 0; e < K; ++e) m[e] = -FLT_MAX;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const long long pix = ((long long)n * H + 2 * y + dy) * W + 2 * x + dx;
      Chunk<T>::unpack(src[pix * nch + ch], v);
#pragma unroll
      for (int e = 0; e < K; ++e) m[e] = fmaxf(m[e], v[e]);
    }
  reinterpret_cast<uint4*>(out)[gid] = Chunk<T>::pack(m);
}

// ------------------------------------------------------------------ spatial attention
// stats[p] = (mean_c x, max_c x); G lanes cooperate on one pixel.
template <typename T>
__global__ void __launch_bounds__(256) attn_stats_kernel(const void* x, long long P, int C, float* stats) {
  constexpr int K = Chunk<T>::N;
  constexpr int G = 16;
  const int nch = C / K;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix = gid / G;
  const int l = (int)(gid % G);
  float s = 0.f, m = -FLT_MAX, v[K];
  if (pix < P) {
    const uint4* src = reinterpret_cast<const uint4*>(x) + pix * nch;
    for (int ch = l; ch < nch; ch += G) {
      Chunk<T>::unpack(src[ch], v);
#pragma unroll
      for (int e = 0; e < K; ++e) { s += v[e]; m = fmaxf(m, v[e]); }
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, G);
    m = fmaxf(m, __shfl_xor(m, off, G));
  }
  if (pix < P && l == 0) {
    stats[pix * 2] = s / (float)C;
    stats[pix * 2 + 1] = m;
  }
}

__global__ void __launch_bounds__(256) attn_map_kernel(const float* stats, int N, int H, int W, const float* w, int k,
                                                       float* att) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)N * H * W;
  if (gid >= total) return;
  const int x = (int)(gid % W);
  const long long t = gid / W;
  const int y = (int)(t % H);
  const int n = (int)(t / H);
  const int r = k / 2;
  float acc = 0.f;
  for (int c = 0; c < 2; ++c)
    for (int ky = 0; ky < k; ++ky) {
      const int yy = y + ky - r;
      if (yy < 0 || yy >= H) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int xx = x + kx - r;
        if (xx < 0 || xx >= W) continue;
        acc += w[(c * k + ky) * k + kx] * stats[(((long long)n * H + yy) * W + xx) * 2 + c];
      }
    }
  att[gid] = sigmoidf_(acc);
}

void attn_map_launch(const float* stats, int N, int H, int W, const float* w7, int k, float* att, hipStream_t s) {
  hipLaunchKernelGGL(attn_map_kernel, dim3(nblocks((long long)N * H * W, 256)), dim3(256), 0, s, stats, N, H, W, w7, k,
                     att);
}

template <typename T>
__global__ void __launch_bounds__(256) pixel_scale_kernel(const void* x, long long P, int C, const float* att, void* out) {
  constexpr int K = Chunk<T>::N;
  const int nch = C / K;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= P * nch) return;
  const float a = att[gid / nch];
  float v[K];
  Chunk<T>::unpack(reinterpret_cast<const uint4*>(x)[gid], v);
#pragma unroll
  for (int e = 0; e < K; ++e) v[e] *= a;
  reinterpret_cast<uint4*>(out)[gid] = Chunk<T>::pack(v);
}

// ------------------------------------------------------------------ input prologue
// (ord_enc / ord_dec, the order-preserving encoding of the maximum: common.h)
__global__ void reset_max_kernel(unsigned* buf) { *buf = 0u; }  // encodes below -FLT_MAX

__global__ void __launch_bounds__(256) image_max_kernel(const float* x, long long n, unsigned* buf) {
  float m = -FLT_MAX;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  long long head = 0;
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {   // 16-B loads, four in flight per thread (scalar: 1 TB/s)
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const long long n4 = n >> 2;
    long long i = gid;
    for (; i + 3 * stride < n4; i += 4 * stride) {
      const float4 a = x4[i], b = x4[i + stride], c = x4[i + 2 * stride], d = x4[i + 3 * stride];
      m = fmaxf(m, fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w))));
      m = fmaxf(m, fmaxf(fmaxf(fmaxf(c.x, c.y), fmaxf(c.z, c.w)), fmaxf(fmaxf(d.x, d.y), fmaxf(d.z, d.w))));
    }
    for (; i < n4; i += stride) {
      const float4 a = x4[i];
      m = fmaxf(m, fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)));
    }
    head = n4 << 2;
  }
  for (long long i = head + gid; i < n; i += stride) m = fmaxf(m, x[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(buf, ord_enc(m));
}

template <typename T>
__global__ void __launch_bounds__(256) input_norm_kernel(const float* x, int B, int C, int H, int W, const unsigned* maxbuf,
                                                         const float* mean, const float* stdv, void* out, int cpad) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)H * W;
  if (gid >= (long long)B * plane) return;
  const long long b = gid / plane, pp = gid % plane;
  const bool div255 = ord_dec(*maxbuf) > 1.0f;
  for (int c = 0; c < cpad; ++c) {
    float v = 0.f;
    if (c < C) {
      v = x[(b * C + c) * plane + pp];
      if (div255) v = __fdiv_rn(v, 255.0f);
      v = __fdiv_rn(__fsub_rn(v, mean[c]), stdv[c]);
    }
    Elem<T>::store(out, gid * cpad + c, v);
  }
}

// ------------------------------------------------------------------ hierarchical combine
// TN2: the target branch's last 1x1 was applied by the producing conv's epilogue (hiseg_conv2d_desc.head2_out):
// tfeat is then f32 [N * 2h * 2w][2], the pixel's (t0, t1); t_w / t_b are not read.
template <typename T, bool TN2 = false>
__global__ void __launch_bounds__(256) hier_combine_kernel(const float* low, int N, int h, int w, const void* tfeat, int Ct,
                                                           const float* ut_w, const float* ut_scale, const float* ut_shift,
                                                           int ut_act, float ut_beta, int ut_ns, const float* u1_w,
                                                           const float* u1_b, const float* t_w, const float* t_b,
                                                           float* logits, float* bgfg, float* tn) {
  __shared__ float s_ut[2 * 32 * 4], s_us[32], s_ush[32], s_u1[64], s_tw[2 * 512];
  const int t = threadIdx.x;
  for (int i = t; i < 256; i += 256) s_ut[i] = ut_w[i];
  if (t < 32 && !ut_ns) { s_us[t] = ut_scale[t]; s_ush[t] = ut_shift[t]; }
  if (t < 64) s_u1[t] = u1_w[t];
  if constexpr (!TN2)
    for (int i = t; i < 2 * Ct; i += 256) s_tw[i] = t_w[i];
  __syncthreads();
  const int H = 2 * h, W = 2 * w;
  const long long gid = (long long)blockIdx.x * 256 + t;
  const long long total = (long long)N * H * W;
  if (gid >= total) return;
  const int X = (int)(gid % W);
  const long long tt = gid / W;
  const int Y = (int)(tt % H);
  const int n = (int)(tt / H);
  const int dy = Y & 1, dx = X & 1;
  const float* lo = low + (((long long)n * h + (Y >> 1)) * w + (X >> 1)) * 2;
  const float l0 = lo[0], l1 = lo[1];
  float b0 = u1_b[0], b1 = u1_b[1];
  // per-sample tables (LayerNorm2d: ut_ns == 32) are read from global memory, the shared fold otherwise
  const float* usc = ut_ns ? ut_scale + (long long)n * ut_ns : s_us;
  const float* ush = ut_ns ? ut_shift + (long long)n * ut_ns : s_ush;
  for (int co = 0; co < 32; ++co) {
    // ConvTranspose2d weight [ci][co][dy][dx]
    float hsum = l0 * s_ut[((0 * 32 + co) * 2 + dy) * 2 + dx] + l1 * s_ut[((1 * 32 + co) * 2 + dy) * 2 + dx];
    hsum = apply_act(hsum * usc[co] + ush[co], ut_act, ut_beta);
    b0 += s_u1[co] * hsum;
    b1 += s_u1[32 + co] * hsum;
  }
  constexpr int K = Chunk<T>::N;
  float t0, t1;
  if constexpr (TN2) {
    const float2 tq = reinterpret_cast<const float2*>(tfeat)[gid];
    t0 = tq.x;
    t1 = tq.y;
  } else {
    t0 = t_b[0];
    t1 = t_b[1];
    float v[K];
    const uint4* tf = reinterpret_cast<const uint4*>(tfeat) + gid * (Ct / K);
    for (int ch = 0; ch < Ct / K; ++ch) {
      Chunk<T>::unpack(tf[ch], v);
      head2_acc<K>(t0, t1, s_tw + ch * K, s_tw + Ct + ch * K, v);
    }
  }
  const float mx = fmaxf(b0, b1);
  const float e0 = __expf(b0 - mx), e1 = __expf(b1 - mx);
  const float pfg = e1 / (e0 + e1);
  const long long plane = (long long)H * W;
  const long long pp = (long long)Y * W + X;
  float* L = logits + (long long)n * 3 * plane + pp;
  L[0] = b0;
  L[plane] = b1 + t0 * pfg;
  L[2 * plane] = b1 + t1 * pfg;
  if (bgfg) {
    float* G = bgfg + (long long)n * 2 * plane + pp;
    G[0] = b0; G[plane] = b1;
  }
  if (tn) {
    float* Tn = tn + (long long)n * 2 * plane + pp;
    Tn[0] = t0; Tn[plane] = t1;
  }
}

// ------------------------------------------------------------------ layout helpers
template <typename T>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const void* in, int N, int H, int W, int C, int cstride, int coff,
                                                           float* out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)H * W;
  const long long total = (long long)N * C * plane;
  if (gid >= total) return;
  const long long pp = gid % plane;
  const long long nc = gid / plane;
  const int c = (int)(nc % C);
  const long long n = nc / C;
  out[gid] = Elem<T>::load(in, (n * plane + pp) * cstride + coff + c);
}

template <typename T>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* in, int N, int C, int H, int W, void* out, int cpad) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)H * W;
  if (gid >= (long long)N * plane) return;
  const long long n = gid / plane, pp = gid % plane;
  for (int c = 0; c < cpad; ++c) Elem<T>::store(out, gid * cpad + c, c < C ? in[(n * C + c) * plane + pp] : 0.f);
}

// ------------------------------------------------------------------ exported-contract masks
__device__ __forceinline__ float p_target(const float* L, long long plane) {
  const float a = L[0], b = L[plane], c = L[2 * plane];
  const float m = fmaxf(a, fmaxf(b, c));
  const float ea = __expf(a - m), eb = __expf(b - m), ec = __expf(c - m);
  return eb / (ea + eb + ec);
}

__global__ void __launch_bounds__(256) instance_mask_kernel(const float* logits, int N, int mh, int mw, int dil, float* inst) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)mh * mw;
  if (gid >= (long long)N * plane) return;
  const long long n = gid / plane, pp = gid % plane;
  const int y = (int)(pp / mw), x = (int)(pp % mw);
  const float* L = logits + n * 3 * plane;
  float l0 = L[pp], l1 = L[plane + pp], l2 = L[2 * plane + pp];
  if (dil > 0) {
    const float p1 = p_target(L + pp, plane);
    float mx = -FLT_MAX;
    for (int yy = y - dil; yy <= y + dil; ++yy)
      for (int xx = x - dil; xx <= x + dil; ++xx)
        if (yy >= 0 && yy < mh && xx >= 0 && xx < mw) mx = fmaxf(mx, p_target(L + (long long)yy * mw + xx, plane));
    if (mx - p1 > 0.1f) l1 += 2.0f;
  }
  // torch.argmax: first index of the maximum
  int cls = 0;
  float best = l0;
  if (l1 > best) { cls = 1; best = l1; }
  if (l2 > best) { cls = 2; }
  inst[gid] = cls == 1 ? 1.f : 0.f;
}

__global__ void __launch_bounds__(256) binary_mask_kernel(const float* u, int cs, long long P, const float* w, const float* b,
                                                          float* out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= P) return;
  const float v = u[gid * cs];
  const float a0 = w[0] * v + b[0], a1 = w[1] * v + b[1];
  const float m = fmaxf(a0, a1);
  const float e0 = __expf(a0 - m), e1 = __expf(a1 - m);
  out[gid] = e0 / (e0 + e1);
}

// ------------------------------------------------------------------ aux-map helpers
__global__ void __launch_bounds__(256) resize_bilinear_kernel(const float* in, int NC, int H, int W, float* out, int Ho,
                                                              int Wo) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)NC * Ho * Wo;
  if (gid >= total) return;
  const int x = (int)(gid % Wo);
  const long long t = gid / Wo;
  const int y = (int)(t % Ho);
  const long long nc = t / Ho;
  const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
  float sy = (y + 0.5f) * sh - 0.5f;
  float sx = (x + 0.5f) * sw - 0.5f;
  sy = sy < 0.f ? 0.f : sy;
  sx = sx < 0.f ? 0.f : sx;
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly = sy - y0, lx = sx - x0;
  const float* p = in + nc * H * W;
  const float v = (1.f - ly) * ((1.f - lx) * p[y0 * W + x0] + lx * p[y0 * W + x1]) +
                  ly * ((1.f - lx) * p[y1 * W + x0] + lx * p[y1 * W + x1]);
  out[gid] = v;
}

__global__ void __launch_bounds__(256) distance_mask_kernel(const float* x, long long n, const float* thr, float* out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  out[gid] = sigmoidf_((x[gid] - thr[0]) * 10.0f);
}

__global__ void __launch_bounds__(256) output_conv_kernel(const float* u, int B, long long plane, const float* w,
                                                          const float* b, float* out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)B * plane) return;
  const long long n = gid / plane, p = gid % plane;
  const float v = u[gid];
  out[(n * 2) * plane + p] = w[0] * v + b[0];
  out[(n * 2 + 1) * plane + p] = w[1] * v + b[1];
}

}  // namespace hiseg

using namespace hiseg;

#define DISPATCH_T(dtype, KERNEL, ...)                                                        \
  do {                                                                                        \
    if ((dtype) == HISEG_BF16) hipLaunchKernelGGL(KERNEL<bf16_t>, __VA_ARGS__);               \
    else if ((dtype) == HISEG_F32) hipLaunchKernelGGL(KERNEL<float>, __VA_ARGS__);            \
    else { hiseg_set_error("unsupported dtype %d", (int)(dtype)); return HISEG_ERR_BAD_DTYPE; } \
  } while (0)

extern "C" int hiseg_maxpool2x2_fwd(int dtype, const void* in, int N, int H, int W, int C, void* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(in && out && N > 0 && H >= 2 && W >= 2 && C > 0, HISEG_ERR_BAD_SHAPE, "maxpool2x2: bad args");
  HISEG_REQUIRE(C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "maxpool2x2: C must be chunk aligned");
  const long long total = (long long)N * (H / 2) * (W / 2) * (C / chunk_of(dtype));
  DISPATCH_T(dtype, maxpool2x2_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, in, N, H, W, C, out);
  return hiseg_check_launch("maxpool2x2");
}

extern "C" int hiseg_attn_spatial_fwd(int dtype, const void* x, int N, int H, int W, int C, const float* w7, int k,
                                      float* stats, float* att, void* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w7 && stats && att && out && N > 0 && H > 0 && W > 0 && C > 0 && k > 0 && (k & 1), HISEG_ERR_BAD_ARG,
                "attn_spatial: bad args");
  HISEG_REQUIRE(C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "attn_spatial: C must be chunk aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long P = (long long)N * H * W;
  DISPATCH_T(dtype, attn_stats_kernel, dim3(nblocks(P * 16, 256)), dim3(256), 0, s, x, P, C, stats);
  attn_map_launch(stats, N, H, W, w7, k, att, s);
  const long long tot = P * (C / chunk_of(dtype));
  DISPATCH_T(dtype, pixel_scale_kernel, dim3(nblocks(tot, 256)), dim3(256), 0, s, x, P, C, att, out);
  return hiseg_check_launch("attn_spatial");
}

extern "C" int hiseg_attn_map_fwd(int dtype, const void* x, int N, int H, int W, int C, const float* w7, int k,
                                  float* stats, float* att, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w7 && stats && att && N > 0 && H > 0 && W > 0 && C > 0 && k > 0 && (k & 1), HISEG_ERR_BAD_ARG,
                "attn_map: bad args");
  HISEG_REQUIRE(C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "attn_map: C must be chunk aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long P = (long long)N * H * W;
  DISPATCH_T(dtype, attn_stats_kernel, dim3(nblocks(P * 16, 256)), dim3(256), 0, s, x, P, C, stats);
  attn_map_launch(stats, N, H, W, w7, k, att, s);
  return hiseg_check_launch("attn_map");
}

extern "C" int hiseg_pixel_scale_fwd(int dtype, const void* x, long long P, int C, const float* att, void* out,
                                     hiseg_stream_t stream) {
  HISEG_REQUIRE(x && att && out && P > 0 && C > 0, HISEG_ERR_BAD_ARG, "pixel_scale: bad args");
  HISEG_REQUIRE(C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "pixel_scale: C must be chunk aligned");
  const long long tot = P * (C / chunk_of(dtype));
  DISPATCH_T(dtype, pixel_scale_kernel, dim3(nblocks(tot, 256)), dim3(256), 0, (hipStream_t)stream, x, P, C, att, out);
  return hiseg_check_launch("pixel_scale");
}

extern "C" int hiseg_image_max_fwd(const float* x, long long n, float* maxbuf, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && maxbuf && n > 0, HISEG_ERR_BAD_ARG, "image_max: bad args");
  hipStream_t s = (hipStream_t)stream;
  unsigned* buf = reinterpret_cast<unsigned*>(maxbuf);
  hipLaunchKernelGGL(reset_max_kernel, dim3(1), dim3(1), 0, s, buf);
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(image_max_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, n, buf);
  return hiseg_check_launch("image_max");
}

extern "C" int hiseg_input_norm_fwd(int dtype, const float* x, int B, int C, int H, int W, const float* maxbuf,
                                    const float* mean, const float* stdv, void* out, int cpad, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && maxbuf && mean && stdv && out && B > 0 && C > 0 && H > 0 && W > 0 && cpad >= C, HISEG_ERR_BAD_ARG,
                "input_norm: bad args");
  const long long total = (long long)B * H * W;
  DISPATCH_T(dtype, input_norm_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, x, B, C, H, W,
             reinterpret_cast<const unsigned*>(maxbuf), mean, stdv, out, cpad);
  return hiseg_check_launch("input_norm");
}

extern "C" int hiseg_hier_combine_fwd(int dtype, const float* low, int N, int h, int w, const void* tfeat, int Ct,
                                      const float* ut_w, const float* ut_scale, const float* ut_shift, int ut_act,
                                      float ut_beta, int ut_per_sample, const float* u1_w, const float* u1_b,
                                      const float* t_w, const float* t_b, float* logits, float* bgfg, float* tn,
                                      hiseg_stream_t stream) {
  HISEG_REQUIRE(low && tfeat && ut_w && ut_scale && ut_shift && u1_w && u1_b && t_w && t_b && logits, HISEG_ERR_BAD_ARG,
                "hier_combine: null pointer");
  HISEG_REQUIRE(N >= 0 && h > 0 && w > 0 && Ct > 0 && Ct <= 512 && Ct % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE,
                "hier_combine: bad shape (Ct %d)", Ct);
  if (N == 0) return HISEG_OK;
  const long long total = (long long)N * 4 * h * w;
  DISPATCH_T(dtype, hier_combine_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, low, N, h, w, tfeat,
             Ct, ut_w, ut_scale, ut_shift, ut_act, ut_beta, ut_per_sample ? 32 : 0, u1_w, u1_b, t_w, t_b, logits, bgfg,
             tn);
  return hiseg_check_launch("hier_combine");
}

extern "C" int hiseg_hier_combine_tn_fwd(const float* low, int N, int h, int w, const float* tn2, const float* ut_w,
                                         const float* ut_scale, const float* ut_shift, int ut_act, float ut_beta,
                                         int ut_per_sample, const float* u1_w, const float* u1_b, float* logits,
                                         float* bgfg, float* tn, hiseg_stream_t stream) {
  HISEG_REQUIRE(low && tn2 && ut_w && ut_scale && ut_shift && u1_w && u1_b && logits, HISEG_ERR_BAD_ARG,
                "hier_combine_tn: null pointer");
  HISEG_REQUIRE(N >= 0 && h > 0 && w > 0 && ((uintptr_t)tn2 & 7) == 0, HISEG_ERR_BAD_SHAPE, "hier_combine_tn: bad shape");
  if (N == 0) return HISEG_OK;
  const long long total = (long long)N * 4 * h * w;
  hipLaunchKernelGGL((hier_combine_kernel<float, true>), dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, low,
                     N, h, w, (const void*)tn2, 0, ut_w, ut_scale, ut_shift, ut_act, ut_beta, ut_per_sample ? 32 : 0, u1_w,
                     u1_b, (const float*)nullptr, (const float*)nullptr, logits, bgfg, tn);
  return hiseg_check_launch("hier_combine_tn");
}

// LayerNorm2d over upsample_bg_fg's ConvTranspose2d(2, 32, 2, s2) output z (model.py:18-38 at
// refinement.py:501-503): per sample n, mean / biased variance of z over (32, 2h, 2w) accumulated in double,
// then the folded tables scale[n][c] = gamma_c * invstd_n, shift[n][c] = beta_c - mean_n * scale[n][c].
// One block per sample: 32 channel lanes x 8 low-pixel rows, 4 children per low pixel.
__global__ void __launch_bounds__(256) ubf_ln_tables_kernel(const float* low, int h, int w, const float* ut_w,
                                                            const float* ut_b, const float* gamma, const float* beta,
                                                            float eps, int fold_bias, float* mean, float* invstd,
                                                            float* scale, float* shift) {
  __shared__ double s1[256], s2[256];
  __shared__ float s_mi[2];
  const int n = blockIdx.x, t = threadIdx.x, c = t & 31, r = t >> 5;
  float wa[4], wb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { wa[q] = ut_w[c * 4 + q]; wb[q] = ut_w[(32 + c) * 4 + q]; }
  const float bc = ut_b ? ut_b[c] : 0.f;
  double a1 = 0.0, a2 = 0.0;
  const int PL = h * w;
  const float* lo = low + (long long)n * PL * 2;
  for (int p = r; p < PL; p += 8) {
    const float l0 = lo[p * 2], l1 = lo[p * 2 + 1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double z = (double)(l0 * wa[q] + l1 * wb[q] + bc);
      a1 += z; a2 += z * z;
    }
  }
  s1[t] = a1; s2[t] = a2;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (t < st) { s1[t] += s1[t + st]; s2[t] += s2[t + st]; }
    __syncthreads();
  }
  if (t == 0) {
    const double M = 128.0 * PL;
    const double m = s1[0] / M;
    double var = s2[0] / M - m * m;
    if (var < 0.0) var = 0.0;
    const float inv = (float)(1.0 / sqrt(var + (double)eps));
    s_mi[0] = (float)m; s_mi[1] = inv;
    if (mean) mean[n] = (float)m;
    if (invstd) invstd[n] = inv;
  }
  __syncthreads();
  if (t < 32) {   // fold_bias: tables for the bias-free ConvTranspose sum of hier_combine_kernel
    const float k = (gamma ? gamma[t] : 1.f) * s_mi[1];
    const float m = fold_bias && ut_b ? s_mi[0] - ut_b[t] : s_mi[0];
    scale[n * 32 + t] = k;
    shift[n * 32 + t] = (beta ? beta[t] : 0.f) - m * k;
  }
}

extern "C" int hiseg_ubf_ln_tables(const float* low, int N, int h, int w, const float* ut_w, const float* ut_b,
                                   const float* gamma, const float* beta, float eps, int fold_bias, float* mean,
                                   float* invstd, float* scale, float* shift, hiseg_stream_t stream) {
  HISEG_REQUIRE(low && ut_w && scale && shift && N >= 0 && h > 0 && w > 0, HISEG_ERR_BAD_ARG, "ubf_ln_tables: bad args");
  if (N == 0) return HISEG_OK;
  hipLaunchKernelGGL(ubf_ln_tables_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, low, h, w, ut_w, ut_b, gamma,
                     beta, eps, fold_bias, mean, invstd, scale, shift);
  return hiseg_check_launch("ubf_ln_tables");
}

extern "C" int hiseg_nhwc_to_nchw_fwd(int dtype, const void* in, int N, int H, int W, int C, int cstride, int coff, float* out,
                                      hiseg_stream_t stream) {
  // coff >= 0: a negative offset satisfied cstride >= coff + C and read in front of the buffer
  HISEG_REQUIRE(in && out && N >= 0 && H >= 0 && W >= 0 && C > 0 && coff >= 0 && cstride >= coff + C, HISEG_ERR_BAD_ARG,
                "nhwc_to_nchw: bad args");
  const long long total = (long long)N * C * H * W;
  if (total == 0) return HISEG_OK;
  DISPATCH_T(dtype, nhwc_to_nchw_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, in, N, H, W, C, cstride,
             coff, out);
  return hiseg_check_launch("nhwc_to_nchw");
}

extern "C" int hiseg_nchw_to_nhwc_fwd(int dtype, const float* in, int N, int C, int H, int W, void* out, int cpad,
                                      hiseg_stream_t stream) {
  HISEG_REQUIRE(in && out && N >= 0 && H >= 0 && W >= 0 && C > 0 && cpad >= C, HISEG_ERR_BAD_ARG, "nchw_to_nhwc: bad args");
  const long long total = (long long)N * H * W;
  if (total == 0) return HISEG_OK;
  DISPATCH_T(dtype, nchw_to_nhwc_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, in, N, C, H, W, out, cpad);
  return hiseg_check_launch("nchw_to_nhwc");
}

extern "C" int hiseg_instance_masks_fwd(const float* logits, int N, int mh, int mw, int dilation, float* instance,
                                        hiseg_stream_t stream) {
  HISEG_REQUIRE(logits && instance && N >= 0 && mh > 0 && mw > 0 && dilation >= 0, HISEG_ERR_BAD_ARG, "instance_masks: bad args");
  const long long total = (long long)N * mh * mw;
  if (total == 0) return HISEG_OK;
  hipLaunchKernelGGL(instance_mask_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, logits, N, mh, mw,
                     dilation, instance);
  return hiseg_check_launch("instance_masks");
}

extern "C" int hiseg_binary_masks_fwd(int dtype, const void* u, int u_cstride, int B, int H, int W, const float* oc_w,
                                      const float* oc_b, float* binary, hiseg_stream_t stream) {
  HISEG_REQUIRE(dtype == HISEG_F32, HISEG_ERR_BAD_DTYPE, "binary_masks: the UNet logit map is f32");
  HISEG_REQUIRE(u && oc_w && oc_b && binary && B > 0 && H > 0 && W > 0 && u_cstride >= 1, HISEG_ERR_BAD_ARG,
                "binary_masks: bad args");
  const long long P = (long long)B * H * W;
  hipLaunchKernelGGL(binary_mask_kernel, dim3(nblocks(P, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float*>(u), u_cstride, P, oc_w, oc_b, binary);
  return hiseg_check_launch("binary_masks");
}

extern "C" int hiseg_resize_bilinear_fwd(const float* in, int NC, int H, int W, float* out, int Ho, int Wo,
                                         hiseg_stream_t stream) {
  HISEG_REQUIRE(in && out && NC >= 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, HISEG_ERR_BAD_ARG, "resize_bilinear: bad args");
  const long long total = (long long)NC * Ho * Wo;
  if (total == 0) return HISEG_OK;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, in, NC, H, W, out,
                     Ho, Wo);
  return hiseg_check_launch("resize_bilinear");
}

extern "C" int hiseg_distance_mask_fwd(const float* x, long long n, const float* threshold, float* out,
                                       hiseg_stream_t stream) {
  HISEG_REQUIRE(x && threshold && out && n >= 0, HISEG_ERR_BAD_ARG, "distance_mask: bad args");
  if (n == 0) return HISEG_OK;
  hipLaunchKernelGGL(distance_mask_kernel, dim3(nblocks(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, threshold, out);
  return hiseg_check_launch("distance_mask");
}

extern "C" int hiseg_output_conv_fwd(const float* u, int B, int H, int W, const float* w, const float* b, float* out,
                                     hiseg_stream_t stream) {
  HISEG_REQUIRE(u && w && b && out && B > 0 && H > 0 && W > 0, HISEG_ERR_BAD_ARG, "output_conv: bad args");
  const long long P = (long long)B * H * W;
  hipLaunchKernelGGL(output_conv_kernel, dim3(nblocks(P, 256)), dim3(256), 0, (hipStream_t)stream, u, B, (long long)H * W, w,
                     b, out);
  return hiseg_check_launch("output_conv");
}

// ------------------------------------------------------------------------------------------ test utility
__global__ void __launch_bounds__(256) debug_fill_lds_kernel(unsigned pattern, int words) {
  extern __shared__ unsigned lds_fill[];
  for (int i = threadIdx.x; i < words; i += 256) lds_fill[i] = pattern;
  __syncthreads();
  // keep the stores: a data-dependent (never true) global write the compiler cannot prove dead
  if (lds_fill[(threadIdx.x * 7) % words] == pattern + 1u && pattern == 0x12345678u) asm volatile("s_nop 0");
}

extern "C" int hiseg_debug_fill_lds(unsigned pattern, int rounds, hiseg_stream_t stream) {
  HISEG_REQUIRE(rounds >= 1 && rounds <= 64, HISEG_ERR_BAD_ARG, "debug_fill_lds: rounds 1..64");
  const int bytes = 160 * 1024;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)debug_fill_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    attr = true;
  }
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  hipLaunchKernelGGL(debug_fill_lds_kernel, dim3(cus * rounds), dim3(256), bytes, (hipStream_t)stream, pattern,
                     bytes / 4);
  return hiseg_check_launch("debug_fill_lds");
}
