// Dropout2d masks with their seed counter, and the element-wise backward passes of the ROI path (gfx950): ReLU,
// sigmoid, gate and activation backwards, in-place add, max-pool, 2x-upsample and bilinear-resize backwards.
// HBM-streaming passes over NHWC activations, f32 arithmetic, storage in the compute dtype.
#include "train_norm.h"

namespace hiseg {

// ---------------------------------------------------------------------------------------- dropout
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ void dropout2d_mask_kernel(int n, float p, unsigned long long seed, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float u = (float)(splitmix64(seed ^ splitmix64((unsigned long long)i)) >> 40) * (1.0f / 16777216.0f);
  out[i] = u < p ? 0.f : 1.f / (1.f - p);
}

// Device-resident seed: seed = (base * 0x9E3779B1 + offset) masked to 48 bits, base read from device memory, so
// a captured step replays with fresh masks once hiseg_seed_advance (captured with it) moved the base on.
__global__ void dropout2d_mask_dev_kernel(int n, float p, const unsigned long long* base, unsigned long long offset,
                                          float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long seed = (base[0] * 0x9E3779B1ull + offset) & 0xFFFFFFFFFFFFull;
  const float u = (float)(splitmix64(seed ^ splitmix64((unsigned long long)i)) >> 40) * (1.0f / 16777216.0f);
  out[i] = u < p ? 0.f : 1.f / (1.f - p);
}

__global__ void seed_advance_kernel(unsigned long long* base) {
  if (threadIdx.x == 0) base[0] += 1ull;
}

// ---------------------------------------------------------------------------------------- element-wise
#define EW_LOOP(P, C)                                                                                   \
  const long long n_ = (P) * (C);                                                                      \
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_; i += (long long)gridDim.x * 256)

__device__ __forceinline__ long long vi(const hiseg_ew_view& v, long long p, int c) { return p * v.cstride + v.coff + c; }

template <typename T>
__global__ void __launch_bounds__(256) relu_bwd_kernel(long long P, int HW, int C, hiseg_ew_view dy, hiseg_ew_view y,
                                                       const float* mul, hiseg_ew_view dz) {
  EW_LOOP(P, C) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    float g = ld<T>(dy.p, vi(dy, p, c));
    if (mul) g *= mul[(p / HW) * C + c];
    st<T>(dz.p, vi(dz, p, c), ld<T>(y.p, vi(y, p, c)) > 0.f ? g : 0.f);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) sigmoid_bwd_kernel(long long P, int C, hiseg_ew_view dy, hiseg_ew_view s,
                                                          hiseg_ew_view dz) {
  EW_LOOP(P, C) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    const float v = ld<T>(s.p, vi(s, p, c));
    st<T>(dz.p, vi(dz, p, c), ld<T>(dy.p, vi(dy, p, c)) * v * (1.f - v));
  }
}

template <typename T>
__global__ void __launch_bounds__(256) gate_fwd_kernel(long long P, int C, hiseg_ew_view a, hiseg_ew_view g,
                                                       hiseg_ew_view out) {
  EW_LOOP(P, C) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    st<T>(out.p, vi(out, p, c), ld<T>(a.p, vi(a, p, c)) * ld<T>(g.p, vi(g, p, c)));
  }
}

template <typename T>
__global__ void __launch_bounds__(256) gate_bwd_kernel(long long P, int C, hiseg_ew_view dy, hiseg_ew_view a,
                                                       hiseg_ew_view g, hiseg_ew_view da, int acc, hiseg_ew_view dzg) {
  EW_LOOP(P, C) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    const float gy = ld<T>(dy.p, vi(dy, p, c));
    const float gv = ld<T>(g.p, vi(g, p, c));
    const float av = ld<T>(a.p, vi(a, p, c));
    if (da.p) {
      const long long o = vi(da, p, c);
      st<T>(da.p, o, acc ? ld<T>(da.p, o) + gy * gv : gy * gv);
    }
    if (dzg.p) st<T>(dzg.p, vi(dzg, p, c), gy * av * gv * (1.f - gv));
  }
}

// Vector form of gate_bwd_kernel: 16-B chunks, (channel chunk, pixel lane) threads as bn_apply_vec_kernel.
template <typename T>
__global__ void __launch_bounds__(256) gate_bwd_vec_kernel(int P, int C, hiseg_ew_view dy, hiseg_ew_view a,
                                                           hiseg_ew_view g, hiseg_ew_view da, int acc,
                                                           hiseg_ew_view dzg) {
  constexpr int V = Chunk<T>::N;
  const int NCH = C / V;
  const int CT = NCH < 256 ? NCH : 256;
  const int R = 256 / CT;
  const int cl = threadIdx.x % CT, r = threadIdx.x / CT;
  const int ch = blockIdx.y * 256 + cl;
  if (r >= R || ch >= NCH) return;
  const int c = ch * V;
  for (int p = blockIdx.x * R + r; p < P; p += gridDim.x * R) {
    float gy[V], gv[V], o[V];
    ldv<T>(dy.p, (long long)p * dy.cstride + dy.coff + c, gy);
    ldv<T>(g.p, (long long)p * g.cstride + g.coff + c, gv);
    if (da.p) {
      const long long off = (long long)p * da.cstride + da.coff + c;
      if (acc) ldv<T>(da.p, off, o);
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = acc ? o[k] + gy[k] * gv[k] : gy[k] * gv[k];
      stv<T>(da.p, off, o);
    }
    if (dzg.p) {
      float av[V];
      ldv<T>(a.p, (long long)p * a.cstride + a.coff + c, av);
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = gy[k] * av[k] * gv[k] * (1.f - gv[k]);
      stv<T>(dzg.p, (long long)p * dzg.cstride + dzg.coff + c, o);
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) act_bwd_cvt_kernel(long long P, int C, hiseg_ew_view dy, hiseg_ew_view y, int act,
                                                          hiseg_ew_view dz, int acc) {
  EW_LOOP(P, C) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    float g = ld<float>(dy.p, vi(dy, p, c));
    if (act != HISEG_ACT_NONE) g *= act_grad(ld<float>(y.p, vi(y, p, c)), act);
    const long long o = vi(dz, p, c);
    st<T>(dz.p, o, acc ? ld<T>(dz.p, o) + g : g);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) add_kernel(long long P, int C, hiseg_ew_view dst, hiseg_ew_view src) {
  EW_LOOP(P, C) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    const long long o = vi(dst, p, c);
    st<T>(dst.p, o, ld<T>(dst.p, o) + ld<T>(src.p, vi(src, p, c)));
  }
}

template <typename T>
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const void* x, int N, int H, int W, int C, const void* dy,
                                                          void* dx, int acc) {
  const int Ho = H / 2, Wo = W / 2;
  const long long n_ = (long long)N * Ho * Wo * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long long q = i / C;
    const int ox = (int)(q % Wo);
    const long long t2 = q / Wo;
    const int oy = (int)(t2 % Ho);
    const long long n = t2 / Ho;
    long long idx[4];
    float best = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      idx[k] = ((n * H + 2 * oy + (k >> 1)) * W + 2 * ox + (k & 1)) * C + c;
      const float v = ld<T>(x, idx[k]);
      if (v > best || v != v) { best = v; arg = k; }
    }
    const float g = ld<T>(dy, q * C + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float add = k == arg ? g : 0.f;
      st<T>(dx, idx[k], acc ? ld<T>(dx, idx[k]) + add : add);
    }
  }
}

// PyTorch bilinear (align_corners=False) source index of output o: max(0, (o+0.5)*scale-0.5).
__device__ __forceinline__ void bl_src(int o, float scale, int in, int& i0, int& i1, float& l1) {
  float s = scale * (o + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - i0;
}

__global__ void __launch_bounds__(256) resize_bwd_kernel(const float* dy, int NC, int h, int w, int H, int W, float* dx) {
  const long long n_ = (long long)NC * h * w;
  const float sh = (float)h / H, sw = (float)w / W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_; i += (long long)gridDim.x * 256) {
    const int ix = (int)(i % w);
    const int iy = (int)((i / w) % h);
    const long long pl = i / ((long long)h * w);
    const int oy_lo = max(0, (int)floorf((iy - 1.5f) / sh)), oy_hi = min(H - 1, (int)ceilf((iy + 1.5f) / sh));
    const int ox_lo = max(0, (int)floorf((ix - 1.5f) / sw)), ox_hi = min(W - 1, (int)ceilf((ix + 1.5f) / sw));
    float acc = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1; float ly;
      bl_src(oy, sh, h, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int x0, x1; float lx;
        bl_src(ox, sw, w, x0, x1, lx);
        const float wx = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
        if (wx != 0.f) acc += wy * wx * dy[(pl * H + oy) * W + ox];
      }
    }
    dx[i] = acc;
  }
}

// dx (+)= 2x2 sum of dy (nearest-x2 upsample backward), one 16-B chunk per thread
template <typename T>
__global__ void __launch_bounds__(256) up2_bwd_kernel(long long N, int h, int w, int C, hiseg_ew_view dy,
                                                      hiseg_ew_view dx, int accumulate) {
  constexpr int V = Chunk<T>::N;
  const int nch = C / V;
  const long long n_el = N * h * w * nch;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % nch);
    const long long q = i / nch;            // low-res pixel
    const int x = (int)(q % w);
    const long long r = q / w;
    const int y = (int)(r % h);
    const long long n = r / h;
    float acc[V], v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long fp = (n * 2 * h + 2 * y + (j >> 1)) * (2 * w) + 2 * x + (j & 1);
      Chunk<T>::unpack(*reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(dy.p) + fp * dy.cstride + dy.coff +
                                                       ch * V), v);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += v[k];
    }
    T* dst = reinterpret_cast<T*>(dx.p) + q * dx.cstride + dx.coff + ch * V;
    if (accumulate) {
      Chunk<T>::unpack(*reinterpret_cast<const uint4*>(dst), v);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += v[k];
    }
    *reinterpret_cast<uint4*>(dst) = Chunk<T>::pack(acc);
  }
}

// dz (+)= dy * act'(z) for an activation applied without normalisation (the fg_gate convs with GELU / Swish /
// SiLU: the conv writes the pre-activation, hiseg_bn_apply with unit tables the activation).
template <typename T>
__global__ void __launch_bounds__(256) act_bwd_pre_kernel(long long P, int C, hiseg_ew_view dy, hiseg_ew_view z, int act,
                                                          float beta, hiseg_ew_view dz, int accumulate) {
  EW_LOOP(P, C) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    float g = ld<T>(dy.p, vi(dy, p, c)) * act_grad_pre(ld<T>(z.p, vi(z, p, c)), act, beta);
    if (accumulate) g += ld<T>(dz.p, vi(dz, p, c));
    st<T>(dz.p, vi(dz, p, c), g);
  }
}
}  // namespace hiseg

using namespace hiseg;

extern "C" int hiseg_dropout2d_mask_dev(int N, int C, float p, const unsigned long long* seed_base,
                                        unsigned long long offset, float* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(seed_base && out && N > 0 && C > 0 && p >= 0.f && p < 1.f, HISEG_ERR_BAD_ARG, "dropout2d_mask_dev: bad args");
  const int n = N * C;
  hipLaunchKernelGGL(dropout2d_mask_dev_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, p,
                     seed_base, offset, out);
  return hiseg_check_launch("dropout2d_mask_dev");
}

extern "C" int hiseg_seed_advance(unsigned long long* seed_base, hiseg_stream_t stream) {
  HISEG_REQUIRE(seed_base, HISEG_ERR_BAD_ARG, "seed_advance: null");
  hipLaunchKernelGGL(seed_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, seed_base);
  return hiseg_check_launch("seed_advance");
}

extern "C" int hiseg_dropout2d_mask(int N, int C, float p, unsigned long long seed, float* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(out && N > 0 && C > 0 && p >= 0.f && p < 1.f, HISEG_ERR_BAD_ARG, "dropout2d_mask: bad arguments");
  const int n = N * C;
  hipLaunchKernelGGL(dropout2d_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, p, seed, out);
  return hiseg_check_launch("dropout2d_mask");
}

extern "C" int hiseg_relu_bwd(int dtype, long long P, int HW, int C, hiseg_ew_view dy, hiseg_ew_view y,
                              const float* chan_mul, hiseg_ew_view dz, hiseg_stream_t stream) {
  HISEG_REQUIRE(dy.p && y.p && dz.p && P > 0 && C > 0 && HW > 0, HISEG_ERR_BAD_ARG, "relu_bwd: bad arguments");
  DISPATCH_T(dtype, hipLaunchKernelGGL(relu_bwd_kernel<T>, dim3(ew_blocks(P * C)), dim3(256), 0, (hipStream_t)stream,
                                       P, HW, C, dy, y, chan_mul, dz));
  return hiseg_check_launch("relu_bwd");
}

extern "C" int hiseg_sigmoid_bwd(int dtype, long long P, int C, hiseg_ew_view dy, hiseg_ew_view s, hiseg_ew_view dz,
                                 hiseg_stream_t stream) {
  HISEG_REQUIRE(dy.p && s.p && dz.p && P > 0 && C > 0, HISEG_ERR_BAD_ARG, "sigmoid_bwd: bad arguments");
  DISPATCH_T(dtype, hipLaunchKernelGGL(sigmoid_bwd_kernel<T>, dim3(ew_blocks(P * C)), dim3(256), 0,
                                       (hipStream_t)stream, P, C, dy, s, dz));
  return hiseg_check_launch("sigmoid_bwd");
}

extern "C" int hiseg_gate_fwd(int dtype, long long P, int C, hiseg_ew_view a, hiseg_ew_view g, hiseg_ew_view out,
                              hiseg_stream_t stream) {
  HISEG_REQUIRE(a.p && g.p && out.p && P > 0 && C > 0, HISEG_ERR_BAD_ARG, "gate_fwd: bad arguments");
  DISPATCH_T(dtype, hipLaunchKernelGGL(gate_fwd_kernel<T>, dim3(ew_blocks(P * C)), dim3(256), 0, (hipStream_t)stream,
                                       P, C, a, g, out));
  return hiseg_check_launch("gate_fwd");
}

extern "C" int hiseg_gate_bwd(int dtype, long long P, int C, hiseg_ew_view dy, hiseg_ew_view a, hiseg_ew_view g,
                              hiseg_ew_view da, int da_accumulate, hiseg_ew_view dzg, hiseg_stream_t stream) {
  HISEG_REQUIRE(dy.p && a.p && g.p && P > 0 && C > 0, HISEG_ERR_BAD_ARG, "gate_bwd: bad arguments");
  if (P < (1ll << 31) && vec_ok(dtype, C, dy.p, dy.cstride, dy.coff) && vec_ok(dtype, C, a.p, a.cstride, a.coff) &&
      vec_ok(dtype, C, g.p, g.cstride, g.coff) && vec_ok(dtype, C, da.p, da.cstride, da.coff) &&
      vec_ok(dtype, C, dzg.p, dzg.cstride, dzg.coff)) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(gate_bwd_vec_kernel<T>, vec_grid(P, C, dtype), dim3(256), 0,
                                         (hipStream_t)stream, (int)P, C, dy, a, g, da, da_accumulate, dzg));
    return hiseg_check_launch("gate_bwd");
  }
  DISPATCH_T(dtype, hipLaunchKernelGGL(gate_bwd_kernel<T>, dim3(ew_blocks(P * C)), dim3(256), 0, (hipStream_t)stream,
                                       P, C, dy, a, g, da, da_accumulate, dzg));
  return hiseg_check_launch("gate_bwd");
}

extern "C" int hiseg_act_bwd_cvt(int dtype, long long P, int C, hiseg_ew_view dy, hiseg_ew_view y, int act,
                                 hiseg_ew_view dz, int accumulate, hiseg_stream_t stream) {
  HISEG_REQUIRE(dy.p && dz.p && P > 0 && C > 0 && (act == HISEG_ACT_NONE || y.p), HISEG_ERR_BAD_ARG,
                "act_bwd_cvt: bad arguments");
  // the derivative is taken from the OUTPUT y: SiLU / GELU / Swish are not functions of it (act_bwd_pre takes them)
  HISEG_REQUIRE(!act_smooth(act), HISEG_ERR_BAD_ARG, "act_bwd_cvt: a smooth activation needs its pre-activation");
  DISPATCH_T(dtype, hipLaunchKernelGGL(act_bwd_cvt_kernel<T>, dim3(ew_blocks(P * C)), dim3(256), 0, (hipStream_t)stream,
                                       P, C, dy, y, act, dz, accumulate));
  return hiseg_check_launch("act_bwd_cvt");
}

extern "C" int hiseg_add_inplace(int dtype, long long P, int C, hiseg_ew_view dst, hiseg_ew_view src,
                                 hiseg_stream_t stream) {
  HISEG_REQUIRE(dst.p && src.p && P > 0 && C > 0, HISEG_ERR_BAD_ARG, "add_inplace: bad arguments");
  DISPATCH_T(dtype, hipLaunchKernelGGL(add_kernel<T>, dim3(ew_blocks(P * C)), dim3(256), 0, (hipStream_t)stream, P, C,
                                       dst, src));
  return hiseg_check_launch("add_inplace");
}

extern "C" int hiseg_maxpool2x2_bwd(int dtype, const void* x, int N, int H, int W, int C, const void* dy, void* dx,
                                    int accumulate, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && dy && dx && N > 0 && H % 2 == 0 && W % 2 == 0 && C > 0, HISEG_ERR_BAD_ARG,
                "maxpool2x2_bwd: bad arguments");
  DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(ew_blocks((long long)N * H * W * C / 4)), dim3(256),
                                       0, (hipStream_t)stream, x, N, H, W, C, dy, dx, accumulate));
  return hiseg_check_launch("maxpool2x2_bwd");
}

extern "C" int hiseg_upsample2x_bwd(int dtype, long long N, int h, int w, int C, hiseg_ew_view dy, hiseg_ew_view dx,
                                    int accumulate, hiseg_stream_t stream) {
  HISEG_REQUIRE(dy.p && dx.p && N > 0 && h > 0 && w > 0 && C > 0, HISEG_ERR_BAD_ARG, "upsample2x_bwd: bad arguments");
  HISEG_REQUIRE(vec_ok(dtype, C, dy.p, dy.cstride, dy.coff) && vec_ok(dtype, C, dx.p, dx.cstride, dx.coff),
                HISEG_ERR_BAD_SHAPE, "upsample2x_bwd: channels/strides must be whole 16-B chunks");
  const long long n = N * h * w * (C / (dtype == HISEG_BF16 ? 8 : 4));
  DISPATCH_T(dtype, hipLaunchKernelGGL(up2_bwd_kernel<T>, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, N, h, w,
                                       C, dy, dx, accumulate));
  return hiseg_check_launch("upsample2x_bwd");
}

extern "C" int hiseg_resize_bilinear_bwd(const float* dy, int NC, int h, int w, int H, int W, float* dx,
                                         hiseg_stream_t stream) {
  HISEG_REQUIRE(dy && dx && NC > 0 && h > 0 && w > 0 && H > 0 && W > 0, HISEG_ERR_BAD_ARG, "resize_bwd: bad arguments");
  hipLaunchKernelGGL(resize_bwd_kernel, dim3(ew_blocks((long long)NC * h * w)), dim3(256), 0, (hipStream_t)stream, dy,
                     NC, h, w, H, W, dx);
  return hiseg_check_launch("resize_bilinear_bwd");
}

extern "C" int hiseg_act_bwd_pre(int dtype, long long P, int C, hiseg_ew_view dy, hiseg_ew_view z, int act,
                                 float act_beta, hiseg_ew_view dz, int accumulate, hiseg_stream_t stream) {
  HISEG_REQUIRE(dy.p && z.p && dz.p && P > 0 && C > 0, HISEG_ERR_BAD_ARG, "act_bwd_pre: bad arguments");
  DISPATCH_T(dtype, hipLaunchKernelGGL(act_bwd_pre_kernel<T>, dim3(ew_blocks(P * C)), dim3(256), 0, (hipStream_t)stream,
                                       P, C, dy, z, act, act_beta, dz, accumulate));
  return hiseg_check_launch("act_bwd_pre");
}
