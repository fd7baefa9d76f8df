// The channel gate in training (gfx950): global average pool -> two-layer MLP -> sigmoid gate -> x * gate, forward and
// backward, for its two users:
//   * ChannelAttentionModule (attention_modules.py:10-64) of the refined head: no biases, Dropout2d table chan_mul
//   * timm SqueezeExcite of the EfficientNet student (effunet_train.py): biases, SiLU, no table
// HBM-streaming kernels; reductions go through deterministic per-block partials (no atomics).
#include "train_norm.h"
#include "hiseg_head_train.h"

namespace hiseg {

// Global-average-pool partials part[n][s][c] over S pixel splits per image, S = ca_splits(N, HW) <= kGapSplits (the
// workspace size).  (Round 5: S was a fixed 16 -- N x 16 blocks, 64 for the distillation student's 4 images -- and
// channel counts whose chunk count does not divide 256 (96, 144, 240, 480, 672, 1152: most SqueezeExcite layers) took
// a one-thread-per-channel kernel with 2-byte loads: the SE forward and backward pools were most of the unfrozen
// distillation step's SE time.)
constexpr int kGapSplits = 64;

static int ca_splits(int N, int HW) {
  int s = 1024 / (N > 0 ? N : 1);
  const int cap = HW / 16 > 0 ? HW / 16 : 1;   // >= 16 pixels per split
  if (s > cap) s = cap;
  if (s > kGapSplits) s = kGapSplits;
  return s < 1 ? 1 : s;
}

// part[n][s][c] = sum_{p in split s of image n} x[p][c] (* dout[p][c] * mul[n][c] if dout).  16-B loads: 256 threads =
// R = 256 / CT pixel lanes x CT channel chunks (CT = min(nch, 256); blockIdx.z: the chunk group), lanes reduced in LDS
// in lane order.
template <typename T>
__global__ void __launch_bounds__(256) ca_gap_vec_kernel(const void* x, const void* dout, const float* mul, int HW,
                                                         int C, int S, float* part) {
  constexpr int K = Chunk<T>::N;
  __shared__ float red[256 * K];   // [R][CT * K]
  const int n = blockIdx.x, sp = blockIdx.y;
  const int nch = C / K;
  const int CT = nch < 256 ? nch : 256, R = 256 / CT;
  const int cl = threadIdx.x % CT, lane = threadIdx.x / CT;
  const int ch = blockIdx.z * 256 + cl;
  const bool live = lane < R && ch < nch;
  const int p0 = (int)((long long)HW * sp / S), p1 = (int)((long long)HW * (sp + 1) / S);
  float acc[K], v[K], g[K];
#pragma unroll
  for (int e = 0; e < K; ++e) acc[e] = 0.f;
  if (live) {
    const uint4* xs = reinterpret_cast<const uint4*>(x) + (long long)n * HW * nch + ch;
    const uint4* ds = dout ? reinterpret_cast<const uint4*>(dout) + (long long)n * HW * nch + ch : nullptr;
    for (int p = p0 + lane; p < p1; p += R) {
      Chunk<T>::unpack(xs[(long long)p * nch], v);
      if (ds) {
        Chunk<T>::unpack(ds[(long long)p * nch], g);
#pragma unroll
        for (int e = 0; e < K; ++e) v[e] *= g[e];
      }
#pragma unroll
      for (int e = 0; e < K; ++e) acc[e] += v[e];
    }
    if (ds && mul) {
#pragma unroll
      for (int e = 0; e < K; ++e) acc[e] *= mul[(long long)n * C + ch * K + e];
    }
  }
  if (lane < R) {
#pragma unroll
    for (int e = 0; e < K; ++e) red[lane * CT * K + cl * K + e] = acc[e];
  }
  __syncthreads();
  const int cols = CT * K;
  for (int c = threadIdx.x; c < cols; c += 256) {
    const int cc = blockIdx.z * 256 * K + c;
    if (cc >= C) continue;
    float s = 0.f;
    for (int l = 0; l < R; ++l) s += red[l * cols + c];
    part[((long long)n * S + sp) * C + cc] = s;
  }
}

template <typename T>
static int ca_gap(const void* x, const void* dout, const float* mul, int N, int HW, int C, float* part, hipStream_t s) {
  const int nch = C / Chunk<T>::N;
  const int S = ca_splits(N, HW);
  hipLaunchKernelGGL(ca_gap_vec_kernel<T>, dim3(N, S, (nch + 255) / 256), dim3(256), 0, s, x, dout, mul, HW, C, S, part);
  return S;
}

__device__ __forceinline__ float act_f(float v, int act, float beta) { return apply_act(v, act, beta); }
__device__ __forceinline__ float act_d(float pre, int act, float beta) { return act_grad_pre(pre, act, beta); }

// out = x * gate[n][c] * mul[n][c]   (NHWC, C channels contiguous).  Block = (256 / nch) pixel lanes x nch
// channel chunks over a pixel range of image blockIdx.y (blockIdx.x = range): the chunk's gate factors stay
// in registers across the thread's pixels.  Falls back to one chunk per thread when nch does not divide 256.
static unsigned ca_ranges(int N, int HW) {   // pixel ranges per image: ~8k blocks, >= 64 pixels per range
  long long r = (8192 + N - 1) / N;
  const long long cap = HW / 64 > 0 ? HW / 64 : 1;
  if (r > cap) r = cap;
  return (unsigned)(r < 1 ? 1 : (r > 65535 ? 65535 : r));
}

template <typename T>
__global__ void __launch_bounds__(256) ca_apply_kernel(const void* x, int N, int HW, int C, const float* gate,
                                                       const float* mul, void* out) {
  constexpr int K = Chunk<T>::N;
  const int nch = C / K;
  const long long n = blockIdx.y;
  if (nch <= 256 && 256 % nch == 0) {
    const int R = 256 / nch, ch = threadIdx.x % nch, lane = threadIdx.x / nch;
    float g[K];
#pragma unroll
    for (int e = 0; e < K; ++e) g[e] = gate[n * C + ch * K + e] * (mul ? mul[n * C + ch * K + e] : 1.f);
    const int p0 = (int)((long long)HW * blockIdx.x / gridDim.x), p1 = (int)((long long)HW * (blockIdx.x + 1) / gridDim.x);
    const uint4* xs = reinterpret_cast<const uint4*>(x) + n * HW * nch + ch;
    uint4* os = reinterpret_cast<uint4*>(out) + n * HW * nch + ch;
    for (int p = p0 + lane; p < p1; p += R) {
      float v[K];
      Chunk<T>::unpack(xs[(long long)p * nch], v);
#pragma unroll
      for (int e = 0; e < K; ++e) v[e] *= g[e];
      os[(long long)p * nch] = Chunk<T>::pack(v);
    }
    return;
  }
  for (int li = blockIdx.x * 256 + threadIdx.x; li < HW * nch; li += gridDim.x * 256) {
    const int ch = li % nch;
    const long long gid = n * HW * nch + li;
    float v[K];
    Chunk<T>::unpack(reinterpret_cast<const uint4*>(x)[gid], v);
    const float* gg = gate + n * C + ch * K;
    const float* m = mul ? mul + n * C + ch * K : nullptr;
#pragma unroll
    for (int e = 0; e < K; ++e) v[e] *= gg[e] * (m ? m[e] : 1.f);
    reinterpret_cast<uint4*>(out)[gid] = Chunk<T>::pack(v);
  }
}

// per image: ds = dgate * g (1-g); dh; dgap; per-image weight-gradient rows
// The channel-attention / SqueezeExcite MLP over the pooled vector, as three wide launches (round 5: one block per
// image did it all -- 4 blocks for the distillation student's SE layers, 45 us forward / 66 us backward per call):
//   colsum:  out[n][c] = (sum_k part[n][k][c]) * HW^-1 (forward: the pool)  or  * g (1 - g) (backward: ds)
//   rowdot:  one 32-lane group per (n, r): s = sum_c W[r ldr + c ldc] v[n][c] (lane-strided, butterfly-reduced)
//            forward: hpre = s + b1, h = act(hpre);  backward: dh = s * act'(hpre)
//   coldot:  one thread per (n, c): s = sum_r W[c ldc + r ldr] v[n][r]
//            forward: gate = sigmoid(s + b2);  backward: dgap = s
__global__ void __launch_bounds__(256) ca_colsum_kernel(const float* part, int S, int C, float inv_hw, const float* gate,
                                                        float* out, int out_ld, int out_off, float* out2) {
  const int n = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float* p = part + (long long)n * S * C + c;
  float s = 0.f;
  int k = 0;
  for (; k + 3 < S; k += 4) {
    const float a0 = p[(long long)k * C], a1 = p[(long long)(k + 1) * C], a2 = p[(long long)(k + 2) * C],
                a3 = p[(long long)(k + 3) * C];
    s += a0; s += a1; s += a2; s += a3;
  }
  for (; k < S; ++k) s += p[(long long)k * C];
  float v;
  if (gate) {
    const float g = gate[(long long)n * C + c];
    v = s * g * (1.f - g);
  } else {
    v = s * inv_hw;
  }
  out[(long long)n * out_ld + out_off + c] = v;
  if (out2) out2[(long long)n * C + c] = v;
}

__global__ void __launch_bounds__(256) ca_rowdot_kernel(const float* W, long long ldr, long long ldc, const float* v,
                                                        int v_ld, int v_off, int C, int Cr, const float* b1, int act,
                                                        float beta, float* hpre, float* out, int out_ld, int fwd) {
  const int n = blockIdx.y, r = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
  float s = 0.f;
  if (r < Cr) {
    const float* vv = v + (long long)n * v_ld + v_off;
    for (int c = l; c < C; c += 32) s += W[r * ldr + c * ldc] * vv[c];
  }
#pragma unroll
  for (int m = 16; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  if (l == 0 && r < Cr) {
    if (fwd) {
      const float pre = s + (b1 ? b1[r] : 0.f);
      hpre[(long long)n * Cr + r] = pre;
      out[(long long)n * out_ld + r] = act_f(pre, act, beta);
    } else {
      out[(long long)n * out_ld + r] = s * act_d(hpre[(long long)n * Cr + r], act, beta);
    }
  }
}

__global__ void __launch_bounds__(256) ca_coldot_kernel(const float* W, long long ldc, long long ldr, const float* v,
                                                        int v_ld, int C, int Cr, const float* b2, int fwd, float* out) {
  const int n = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float* vv = v + (long long)n * v_ld;
  float s = 0.f;
  for (int r = 0; r < Cr; ++r) s += W[c * ldc + r * ldr] * vv[r];
  out[(long long)n * C + c] = fwd ? sigmoidf_(s + (b2 ? b2[c] : 0.f)) : s;
}

// forward: gap [N][C], hpre [N][Cr], gate [N][C]; h [N][Cr] in scratch
static void ca_mlp_fwd(const float* part, int S, int N, int HW, int C, int Cr, const float* w1, const float* w2, int act,
                       float beta, float* gap, float* hpre, float* gate, const float* b1, const float* b2, float* h,
                       hipStream_t s) {
  const dim3 cg((C + 255) / 256, N), rg((Cr + 7) / 8, N);
  hipLaunchKernelGGL(ca_colsum_kernel, cg, dim3(256), 0, s, part, S, C, 1.f / (float)HW, nullptr, gap, C, 0, nullptr);
  hipLaunchKernelGGL(ca_rowdot_kernel, rg, dim3(256), 0, s, w1, (long long)C, 1ll, gap, C, 0, C, Cr, b1, act, beta, hpre,
                     h, Cr, 1);
  hipLaunchKernelGGL(ca_coldot_kernel, cg, dim3(256), 0, s, w2, (long long)Cr, 1ll, h, Cr, C, Cr, b2, 1, gate);
}

// backward: sd [N][Cr + C] = (dh, ds), dgap [N][C]
static void ca_mlp_bwd(const float* part, int S, int N, int C, int Cr, const float* w1, const float* w2, int act,
                       float beta, const float* hpre, const float* gate, float* dgap, float* sd, hipStream_t s) {
  const dim3 cg((C + 255) / 256, N), rg((Cr + 7) / 8, N);
  hipLaunchKernelGGL(ca_colsum_kernel, cg, dim3(256), 0, s, part, S, C, 0.f, gate, sd, Cr + C, Cr, nullptr);
  hipLaunchKernelGGL(ca_rowdot_kernel, rg, dim3(256), 0, s, w2, 1ll, (long long)Cr, sd, Cr + C, Cr, C, Cr, nullptr, act,
                     beta, const_cast<float*>(hpre), sd, Cr + C, 0);
  hipLaunchKernelGGL(ca_coldot_kernel, cg, dim3(256), 0, s, w1, 1ll, (long long)C, sd, Cr + C, C, Cr, nullptr, 0, dgap);
}

// dW1[r][c] += sum_n dh[n][r] gap[n][c]; dW2[c][r] += sum_n ds[n][c] act(hpre[n][r]); db1 += sum_n dh; db2 += sum_n ds
// (images in order).  One thread per output element over many blocks -- the per-image rows were written by one block
// per image and summed by four more launches (the distillation student's SE layers: 4 blocks for up to 2 x 55 k
// outputs).
__global__ void __launch_bounds__(256) ca_wgrad_kernel(int N, int C, int Cr, const float* sd, const float* gap,
                                                       const float* hpre, int act, float beta, float* dw1, float* dw2,
                                                       float* db1, float* db2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n1 = (long long)C * Cr;
  const int ld = Cr + C;
  if (i < n1) {
    const int r = (int)(i / C), c = (int)(i - (long long)r * C);
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += sd[(long long)n * ld + r] * gap[(long long)n * C + c];
    dw1[i] += s;
  } else if (i < 2 * n1) {
    const long long j = i - n1;
    const int c = (int)(j / Cr), r = (int)(j - (long long)c * Cr);
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += sd[(long long)n * ld + Cr + c] * act_f(hpre[(long long)n * Cr + r], act, beta);
    dw2[j] += s;
  } else if (i < 2 * n1 + Cr) {
    const int r = (int)(i - 2 * n1);
    if (db1) {
      float s = 0.f;
      for (int n = 0; n < N; ++n) s += sd[(long long)n * ld + r];
      db1[r] += s;
    }
  } else if (i < 2 * n1 + Cr + C) {
    const int c = (int)(i - 2 * n1 - Cr);
    if (db2) {
      float s = 0.f;
      for (int n = 0; n < N; ++n) s += sd[(long long)n * ld + Cr + c];
      db2[c] += s;
    }
  }
}

static void ca_wgrad(int N, int C, int Cr, const float* sd, const float* gap, const float* hpre, int act, float beta,
                     float* dw1, float* dw2, float* db1, float* db2, hipStream_t s) {
  const long long n = 2ll * C * Cr + Cr + C;
  hipLaunchKernelGGL(ca_wgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, N, C, Cr, sd, gap, hpre, act,
                     beta, dw1, dw2, db1, db2);
}

// dx = dout*mul*gate + dgap/HW, same block layout as ca_apply_kernel
template <typename T>
__global__ void __launch_bounds__(256) ca_dx_kernel(const void* dout, int N, int HW, int C, const float* gate,
                                                    const float* mul, const float* dgap, void* dx) {
  constexpr int K = Chunk<T>::N;
  const int nch = C / K;
  const long long n = blockIdx.y;
  const float inv = 1.f / (float)HW;
  if (nch <= 256 && 256 % nch == 0) {
    const int R = 256 / nch, ch = threadIdx.x % nch, lane = threadIdx.x / nch;
    float g[K], d[K];
#pragma unroll
    for (int e = 0; e < K; ++e) {
      const long long i = n * C + ch * K + e;
      g[e] = gate[i] * (mul ? mul[i] : 1.f);
      d[e] = dgap[i] * inv;
    }
    const int p0 = (int)((long long)HW * blockIdx.x / gridDim.x), p1 = (int)((long long)HW * (blockIdx.x + 1) / gridDim.x);
    const uint4* ds = reinterpret_cast<const uint4*>(dout) + n * HW * nch + ch;
    uint4* os = reinterpret_cast<uint4*>(dx) + n * HW * nch + ch;
    for (int p = p0 + lane; p < p1; p += R) {
      float v[K];
      Chunk<T>::unpack(ds[(long long)p * nch], v);
#pragma unroll
      for (int e = 0; e < K; ++e) v[e] = v[e] * g[e] + d[e];
      os[(long long)p * nch] = Chunk<T>::pack(v);
    }
    return;
  }
  for (int li = blockIdx.x * 256 + threadIdx.x; li < HW * nch; li += gridDim.x * 256) {
    const int ch = li % nch;
    const long long gid = n * HW * nch + li;
    float v[K];
    Chunk<T>::unpack(reinterpret_cast<const uint4*>(dout)[gid], v);
#pragma unroll
    for (int e = 0; e < K; ++e) {
      const long long i = n * C + ch * K + e;
      v[e] = v[e] * gate[i] * (mul ? mul[i] : 1.f) + dgap[i] * inv;
    }
    reinterpret_cast<uint4*>(dx)[gid] = Chunk<T>::pack(v);
  }
}

// The workspace of one call, as float offsets into ws (host only):
//   part  [N][kGapSplits][C]   the pool's split partials, forward and backward
//   dgap  [N][C]               backward: d gap; the forward keeps its hidden row h [N][Cr] here
//   wpart [N][2 C Cr]          the per-image weight-gradient region
//   sd    [N][Cr + C]          backward: (dh, ds) rows.  Without biases (channel attention) they live at the start of
//                              wpart; with biases (SqueezeExcite) in a region of their own after it
struct CaPlan { long long dgap, wpart, sd, total; };   // part is at 0

static CaPlan ca_plan(int N, int C, int Cr, bool with_bias) {
  CaPlan p;
  p.dgap = (long long)N * kGapSplits * C;
  p.wpart = p.dgap + (long long)N * C;
  const long long wend = p.wpart + (long long)N * 2 * C * Cr;
  p.sd = with_bias ? wend : p.wpart;
  p.total = with_bias ? wend + (long long)N * (Cr + C) : wend;
  return p;
}

// pool -> MLP (b1, b2 may be null) -> out = x * gate * chan_mul (chan_mul may be null)
static void ca_train_fwd(int dtype, const void* x, int N, int HW, int C, const float* w1, const float* b1, int Cr,
                         const float* w2, const float* b2, int act, float act_beta, const float* chan_mul, float* ws,
                         const CaPlan& p, float* gap, float* hpre, float* gate, void* out, hipStream_t s) {
  int S = 0;
  DISPATCH_T(dtype, S = ca_gap<T>(x, nullptr, nullptr, N, HW, C, ws, s));
  ca_mlp_fwd(ws, S, N, HW, C, Cr, w1, w2, act, act_beta, gap, hpre, gate, b1, b2, ws + p.dgap, s);
  DISPATCH_T(dtype, hipLaunchKernelGGL(ca_apply_kernel<T>, dim3(ca_ranges(N, HW), N),
                                       dim3(256), 0, s, x, N, HW, C, gate, chan_mul, out));
}

// pool of x * dout * chan_mul -> MLP backward -> weight (and, where db1 / db2 are given, bias) gradients -> dx
static void ca_train_bwd(int dtype, const void* x, int N, int HW, int C, const float* w1, int Cr, const float* w2,
                         int act, float act_beta, const float* chan_mul, const float* gap, const float* hpre,
                         const float* gate, const void* dout, void* dx, float* ws, const CaPlan& p, float* dw1,
                         float* db1, float* dw2, float* db2, hipStream_t s) {
  float* dgap = ws + p.dgap;
  float* sd = ws + p.sd;
  int S = 0;
  DISPATCH_T(dtype, S = ca_gap<T>(x, dout, chan_mul, N, HW, C, ws, s));
  ca_mlp_bwd(ws, S, N, C, Cr, w1, w2, act, act_beta, hpre, gate, dgap, sd, s);
  ca_wgrad(N, C, Cr, sd, gap, hpre, act, act_beta, dw1, dw2, db1, db2, s);
  DISPATCH_T(dtype, hipLaunchKernelGGL(ca_dx_kernel<T>, dim3(ca_ranges(N, HW), N),
                                       dim3(256), 0, s, dout, N, HW, C, gate, chan_mul, dgap, dx));
}

}  // namespace hiseg

using namespace hiseg;

extern "C" int hiseg_attn_channel_ws(int N, int C, int Cr) { return (int)ca_plan(N, C, Cr, false).total; }

extern "C" int hiseg_attn_channel_train_fwd(int dtype, const void* x, int N, int HW, int C, const float* w1, int Cr,
                                            const float* w2, int act, float act_beta, const float* chan_mul, float* ws,
                                            float* gap, float* hpre, float* gate, void* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w1 && w2 && ws && gap && hpre && gate && out && N > 0 && HW > 0 && Cr > 0, HISEG_ERR_BAD_ARG,
                "attn_channel_train_fwd: bad args");
  HISEG_REQUIRE(C > 0 && C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "attn_channel_train_fwd: C alignment");
  ca_train_fwd(dtype, x, N, HW, C, w1, nullptr, Cr, w2, nullptr, act, act_beta, chan_mul, ws, ca_plan(N, C, Cr, false),
               gap, hpre, gate, out, (hipStream_t)stream);
  return hiseg_check_launch("attn_channel_train_fwd");
}

extern "C" int hiseg_attn_channel_bwd(int dtype, const void* x, int N, int HW, int C, const float* w1, int Cr,
                                      const float* w2, int act, float act_beta, const float* chan_mul,
                                      const float* gap, const float* hpre, const float* gate, const void* dout, void* dx,
                                      float* ws, float* dw1, float* dw2, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w1 && w2 && gap && hpre && gate && dout && dx && ws && dw1 && dw2, HISEG_ERR_BAD_ARG,
                "attn_channel_bwd: null");
  HISEG_REQUIRE(C > 0 && C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "attn_channel_bwd: C alignment");
  ca_train_bwd(dtype, x, N, HW, C, w1, Cr, w2, act, act_beta, chan_mul, gap, hpre, gate, dout, dx, ws,
               ca_plan(N, C, Cr, false), dw1, nullptr, dw2, nullptr, (hipStream_t)stream);
  return hiseg_check_launch("attn_channel_bwd");
}

// timm SqueezeExcite (EfficientNet MBConv: GAP -> conv_reduce + bias -> SiLU -> conv_expand + bias -> sigmoid)
// in train mode: the channel-attention kernels with biases.  fwd writes gap / hpre / gate and out = x * gate
// (the projection conv's input, materialised so its weight gradient sees it); bwd from d(out).
extern "C" long long hiseg_se_train_ws(int N, int C, int Cr) { return ca_plan(N, C, Cr, true).total; }

extern "C" int hiseg_se_train_fwd(int dtype, const void* x, int N, int HW, int C, const float* w1, const float* b1,
                                  int Cr, const float* w2, const float* b2, int act, float* ws, float* gap,
                                  float* hpre, float* gate, void* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w1 && b1 && w2 && b2 && ws && gap && hpre && gate && out && N > 0 && HW > 0 && Cr > 0,
                HISEG_ERR_BAD_ARG, "se_train_fwd: bad args");
  HISEG_REQUIRE(C > 0 && C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "se_train_fwd: C alignment");
  ca_train_fwd(dtype, x, N, HW, C, w1, b1, Cr, w2, b2, act, 1.f, nullptr, ws, ca_plan(N, C, Cr, true), gap, hpre, gate,
               out, (hipStream_t)stream);
  return hiseg_check_launch("se_train_fwd");
}

extern "C" int hiseg_se_train_bwd(int dtype, const void* x, int N, int HW, int C, const float* w1, int Cr,
                                  const float* w2, int act, const float* gap, const float* hpre, const float* gate,
                                  const void* dout, void* dx, float* ws, float* dw1, float* db1, float* dw2, float* db2,
                                  hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w1 && w2 && gap && hpre && gate && dout && dx && ws && dw1 && db1 && dw2 && db2,
                HISEG_ERR_BAD_ARG, "se_train_bwd: null");
  HISEG_REQUIRE(C > 0 && C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "se_train_bwd: C alignment");
  ca_train_bwd(dtype, x, N, HW, C, w1, Cr, w2, act, 1.f, nullptr, gap, hpre, gate, dout, dx, ws,
               ca_plan(N, C, Cr, true), dw1, db1, dw2, db2, (hipStream_t)stream);
  return hiseg_check_launch("se_train_bwd");
}
