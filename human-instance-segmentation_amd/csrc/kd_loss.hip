// Knowledge-distillation term of the ROI model, forward and backward (include/hiseg_kd.h) on gfx950.
//
// Both passes are HBM streams over the seven student and seven teacher channel planes of a pixel (3 + 2 + 2):
// 14 floats read per pixel forward, 14 read and 7 written backward, one launch for the three heads.  Threads run
// along the pixel axis of one sample, so every channel plane is read coalesced.  A block owns one contiguous range
// of one sample's pixels; its three head sums are reduced by wave64 shuffles, then across the block's four waves
// in a fixed order, and stored as one partial per head.  A one-block finalize kernel adds the partials in a fixed
// order in double.  No atomics.
//
// 16-byte loads are used only when H*W is a multiple of 4 and every base pointer is 16-byte aligned, which makes
// every channel plane 16-byte aligned; otherwise (odd H*W with C = 3 or 2 puts the planes at any 4-byte offset)
// the scalar instantiation runs.
#include <math.h>

#include "common.h"
#include "hiseg_kd.h"

namespace hiseg {

constexpr int kKdThreads = 256;
constexpr int kKdMaxSplits = 64;           // blocks per sample, at most
constexpr long long kKdPixPerBlock = 1024; // pixels per block below that cap (4 per thread)
constexpr float kKdW0 = 1.0f, kKdW1 = 0.3f, kKdW2 = 0.3f;

struct KdArgs {
  const float* s[3];
  const float* t[3];
  float* d[3];          // backward only
  long long HW;
  int N, S;
  float T;
  const float* dev_T;
  const float* gscale;  // backward only
};

static int kd_splits(long long HW) {
  long long s = (HW + kKdPixPerBlock - 1) / kKdPixPerBlock;
  return (int)(s < 1 ? 1 : (s > kKdMaxSplits ? kKdMaxSplits : s));
}

template <int V> struct KdVec;
template <> struct KdVec<1> { using type = float; };
template <> struct KdVec<4> { using type = float4; };

template <int V> __device__ __forceinline__ void kd_load(const float* p, float (&v)[V]);
template <> __device__ __forceinline__ void kd_load<1>(const float* p, float (&v)[1]) { v[0] = p[0]; }
template <> __device__ __forceinline__ void kd_load<4>(const float* p, float (&v)[4]) {
  const float4 x = *reinterpret_cast<const float4*>(p);
  v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
template <int V> __device__ __forceinline__ void kd_store(float* p, const float (&v)[V]);
template <> __device__ __forceinline__ void kd_store<1>(float* p, const float (&v)[1]) { p[0] = v[0]; }
template <> __device__ __forceinline__ void kd_store<4>(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// Student softmax numerators es (sum ss, a_c - max in am) and teacher's (et, st, bm) of one pixel.
template <int C>
__device__ __forceinline__ void kd_softmaxes(const float (&s)[C], const float (&t)[C], float invT, float (&am)[C],
                                             float (&es)[C], float& ss, float (&bm)[C], float (&et)[C], float& st) {
  float ma = s[0] * invT, mb = t[0] * invT;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    am[c] = s[c] * invT;
    bm[c] = t[c] * invT;
    ma = fmaxf(ma, am[c]);
    mb = fmaxf(mb, bm[c]);
  }
  ss = 0.f;
  st = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    am[c] -= ma;
    bm[c] -= mb;
    es[c] = expf(am[c]);
    et[c] = expf(bm[c]);
    ss += es[c];
    st += et[c];
  }
}

// sum_c xlogy(q, q) - q * ls of one pixel
template <int C>
__device__ __forceinline__ float kd_pixel(const float (&s)[C], const float (&t)[C], float invT) {
  float am[C], es[C], bm[C], et[C], ss, st;
  kd_softmaxes<C>(s, t, invT, am, es, ss, bm, et, st);
  const float lss = logf(ss), rst = 1.f / st;
  float r = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float q = et[c] * rst;
    if (q > 0.f) r += q * (logf(q) - (am[c] - lss));
  }
  return r;
}

template <int C>
__device__ __forceinline__ void kd_pixel_grad(const float (&s)[C], const float (&t)[C], float invT, float coef,
                                              float (&g)[C]) {
  float am[C], es[C], bm[C], et[C], ss, st;
  kd_softmaxes<C>(s, t, invT, am, es, ss, bm, et, st);
  const float rss = 1.f / ss, rst = 1.f / st;
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = coef * (es[c] * rss - et[c] * rst);
}

// V consecutive pixels starting at pixel i of the sample whose planes start at sb / tb
template <int C, int V>
__device__ __forceinline__ float kd_head_sum(const float* sb, const float* tb, long long HW, long long i, float invT) {
  float sv[C][V], tv[C][V];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    kd_load<V>(sb + c * HW + i, sv[c]);
    kd_load<V>(tb + c * HW + i, tv[c]);
  }
  float r = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float s[C], t[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { s[c] = sv[c][j]; t[c] = tv[c][j]; }
    r += kd_pixel<C>(s, t, invT);
  }
  return r;
}

template <int C, int V>
__device__ __forceinline__ void kd_head_grad(const float* sb, const float* tb, float* db, long long HW, long long i,
                                             float invT, float coef) {
  float sv[C][V], tv[C][V], gv[C][V];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    kd_load<V>(sb + c * HW + i, sv[c]);
    kd_load<V>(tb + c * HW + i, tv[c]);
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float s[C], t[C], g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { s[c] = sv[c][j]; t[c] = tv[c][j]; }
    kd_pixel_grad<C>(s, t, invT, coef, g);
#pragma unroll
    for (int c = 0; c < C; ++c) gv[c][j] = g[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) kd_store<V>(db + c * HW + i, gv[c]);
}

__device__ __forceinline__ float kd_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// grid: N * S blocks; block b: sample b / S, pixel units [units * sp / S, units * (sp + 1) / S) of V pixels each
template <int V>
__global__ void __launch_bounds__(kKdThreads) kd_fwd_kernel(KdArgs a, float* ws) {
  __shared__ float red[3][kKdThreads / 64];
  const int tid = threadIdx.x;
  const long long n = blockIdx.x / a.S;
  const int sp = blockIdx.x % a.S;
  const long long HW = a.HW, units = HW / V;
  const long long beg = units * sp / a.S, end = units * (sp + 1) / a.S;
  const float invT = 1.f / (a.dev_T ? a.dev_T[0] : a.T);
  float acc[3] = {0.f, 0.f, 0.f};
  for (long long u = beg + tid; u < end; u += kKdThreads) {
    const long long i = u * V;
    if (a.s[0]) acc[0] += kd_head_sum<3, V>(a.s[0] + n * 3 * HW, a.t[0] + n * 3 * HW, HW, i, invT);
    if (a.s[1]) acc[1] += kd_head_sum<2, V>(a.s[1] + n * 2 * HW, a.t[1] + n * 2 * HW, HW, i, invT);
    if (a.s[2]) acc[2] += kd_head_sum<2, V>(a.s[2] + n * 2 * HW, a.t[2] + n * 2 * HW, HW, i, invT);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float w = kd_wave_sum(acc[k]);
    if ((tid & 63) == 0) red[k][tid >> 6] = w;
  }
  __syncthreads();
  if (tid < 3) {
    float r = red[tid][0];
#pragma unroll
    for (int w = 1; w < kKdThreads / 64; ++w) r += red[tid][w];
    ws[(long long)blockIdx.x * 3 + tid] = r;
  }
}

// One block: thread t adds the partials t, t + 256, ... of each head in double, then a fixed-order tree.
__global__ void __launch_bounds__(kKdThreads) kd_finalize_kernel(KdArgs a, const float* ws, float* out) {
  __shared__ double red[3][kKdThreads];
  const int tid = threadIdx.x;
  const long long nb = (long long)a.N * a.S;
  double acc[3] = {0.0, 0.0, 0.0};
  for (long long b = tid; b < nb; b += kKdThreads) {
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += (double)ws[b * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k][tid] = acc[k];
  __syncthreads();
  for (int w = kKdThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double T = a.dev_T ? a.dev_T[0] : a.T;
    const double f = T * T / (double)a.N;
    const double t0 = a.s[0] ? (double)kKdW0 * f * red[0][0] : 0.0;
    const double t1 = a.s[1] ? (double)kKdW1 * f * red[1][0] : 0.0;
    const double t2 = a.s[2] ? (double)kKdW2 * f * red[2][0] : 0.0;
    out[0] = (float)(t0 + t1 + t2);
    out[1] = (float)t0;
    out[2] = (float)t1;
    out[3] = (float)t2;
  }
}

template <int V>
__global__ void __launch_bounds__(kKdThreads) kd_bwd_kernel(KdArgs a) {
  const int tid = threadIdx.x;
  const long long n = blockIdx.x / a.S;
  const int sp = blockIdx.x % a.S;
  const long long HW = a.HW, units = HW / V;
  const long long beg = units * sp / a.S, end = units * (sp + 1) / a.S;
  const float T = a.dev_T ? a.dev_T[0] : a.T;
  const float invT = 1.f / T;
  const float base = a.gscale[0] * (T / (float)a.N);
  const float c0 = base * kKdW0, c1 = base * kKdW1, c2 = base * kKdW2;
  for (long long u = beg + tid; u < end; u += kKdThreads) {
    const long long i = u * V;
    if (a.s[0])
      kd_head_grad<3, V>(a.s[0] + n * 3 * HW, a.t[0] + n * 3 * HW, a.d[0] + n * 3 * HW, HW, i, invT, c0);
    if (a.s[1])
      kd_head_grad<2, V>(a.s[1] + n * 2 * HW, a.t[1] + n * 2 * HW, a.d[1] + n * 2 * HW, HW, i, invT, c1);
    if (a.s[2])
      kd_head_grad<2, V>(a.s[2] + n * 2 * HW, a.t[2] + n * 2 * HW, a.d[2] + n * 2 * HW, HW, i, invT, c2);
  }
}

static bool kd_wide_ok(const KdArgs& a) {
  if (a.HW % 4 != 0) return false;
  for (int k = 0; k < 3; ++k)
    if (!al16(a.s[k]) || !al16(a.t[k]) || !al16(a.d[k])) return false;
  return true;
}

}  // namespace hiseg

using namespace hiseg;

extern "C" long long hiseg_kd_ws(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (long long)N * kd_splits((long long)H * W) * 3 + 1;
}

static int kd_fill(KdArgs& a, const char* what, const float* s0, const float* t0, const float* s1, const float* t1,
                   const float* s2, const float* t2, int N, int H, int W, float T, const float* dev_T) {
  HISEG_REQUIRE(N > 0 && H > 0 && W > 0, HISEG_ERR_BAD_ARG, "%s: bad shape", what);
  HISEG_REQUIRE(!s0 || t0, HISEG_ERR_BAD_ARG, "%s: student logits without teacher logits", what);
  HISEG_REQUIRE((s1 == nullptr) == (t1 == nullptr) && (s2 == nullptr) == (t2 == nullptr), HISEG_ERR_BAD_ARG,
                "%s: an aux head needs its student and its teacher tensor", what);
  HISEG_REQUIRE(dev_T || T > 0.f, HISEG_ERR_BAD_ARG, "%s: temperature must be > 0", what);
  a.HW = (long long)H * W;
  a.N = N;
  a.S = kd_splits(a.HW);
  HISEG_REQUIRE((long long)N * a.S <= 0x7fffffffLL, HISEG_ERR_BAD_SHAPE, "%s: too many samples", what);
  a.s[0] = s0; a.t[0] = s0 ? t0 : nullptr;
  a.s[1] = s1; a.t[1] = t1;
  a.s[2] = s2; a.t[2] = t2;
  a.d[0] = a.d[1] = a.d[2] = nullptr;
  a.T = T;
  a.dev_T = dev_T;
  a.gscale = nullptr;
  return HISEG_OK;
}

extern "C" int hiseg_kd_loss_fwd(const float* s_logits, const float* t_logits, const float* s_bgfg,
                                 const float* t_bgfg, const float* s_tn, const float* t_tn, int N, int H, int W,
                                 float T, const float* dev_T, float* ws, float* out, hiseg_stream_t stream) {
  KdArgs a;
  const int st = kd_fill(a, "kd_loss_fwd", s_logits, t_logits, s_bgfg, t_bgfg, s_tn, t_tn, N, H, W, T, dev_T);
  if (st != HISEG_OK) return st;
  HISEG_REQUIRE(ws && out, HISEG_ERR_BAD_ARG, "kd_loss_fwd: ws and out are required");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((long long)N * a.S));
  if (kd_wide_ok(a))
    hipLaunchKernelGGL(kd_fwd_kernel<4>, grid, dim3(kKdThreads), 0, s, a, ws);
  else
    hipLaunchKernelGGL(kd_fwd_kernel<1>, grid, dim3(kKdThreads), 0, s, a, ws);
  hipLaunchKernelGGL(kd_finalize_kernel, dim3(1), dim3(kKdThreads), 0, s, a, ws, out);
  return hiseg_check_launch("kd_loss_fwd");
}

extern "C" int hiseg_kd_loss_bwd(const float* s_logits, const float* t_logits, const float* s_bgfg,
                                 const float* t_bgfg, const float* s_tn, const float* t_tn, int N, int H, int W,
                                 float T, const float* dev_T, const float* gscale, float* d_logits, float* d_bgfg,
                                 float* d_tn, hiseg_stream_t stream) {
  KdArgs a;
  const int st = kd_fill(a, "kd_loss_bwd", s_logits, t_logits, s_bgfg, t_bgfg, s_tn, t_tn, N, H, W, T, dev_T);
  if (st != HISEG_OK) return st;
  HISEG_REQUIRE(gscale, HISEG_ERR_BAD_ARG, "kd_loss_bwd: gscale is required");
  HISEG_REQUIRE((!s_logits || d_logits) && (!s_bgfg || d_bgfg) && (!s_tn || d_tn), HISEG_ERR_BAD_ARG,
                "kd_loss_bwd: every enabled head needs its gradient tensor");
  a.d[0] = s_logits ? d_logits : nullptr;
  a.d[1] = s_bgfg ? d_bgfg : nullptr;
  a.d[2] = s_tn ? d_tn : nullptr;
  a.gscale = gscale;
  if (!a.s[0] && !a.s[1] && !a.s[2]) return HISEG_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((long long)N * a.S));
  if (kd_wide_ok(a))
    hipLaunchKernelGGL(kd_bwd_kernel<4>, grid, dim3(kKdThreads), 0, s, a);
  else
    hipLaunchKernelGGL(kd_bwd_kernel<1>, grid, dim3(kKdThreads), 0, s, a);
  return hiseg_check_launch("kd_loss_bwd");
}
