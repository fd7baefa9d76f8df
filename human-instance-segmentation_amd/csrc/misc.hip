// Memory-bound kernels of the hot path (pool, attention gates, depthwise conv, layout and
// epilogue kernels).  All are vectorised on 16-B chunks of the NHWC channel dimension
// (cdna_hip_programming.md Guideline 13) and grid-sized for 256 CUs.
#include <float.h>
#include "common.h"
#include "gfx950_prims.h"
#include "head2.h"

namespace hiseg {

static inline unsigned nblocks(long long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

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

// ------------------------------------------------------------------ GAP + SE gate
template <typename T>
__global__ void __launch_bounds__(256) gap_partial_kernel(const void* x, int HW, int C, int splits, float* partial) {
  constexpr int K = Chunk<T>::N;
  extern __shared__ __attribute__((aligned(16))) float red[];
  const int n = blockIdx.x;
  const int sp = blockIdx.y;
  const int nch = C / K;
  const int p0 = (int)((long long)HW * sp / splits), p1 = (int)((long long)HW * (sp + 1) / splits);
  const uint4* src = reinterpret_cast<const uint4*>(x) + (long long)n * HW * nch;
  const int t = threadIdx.x;
  float* out = partial + ((long long)n * splits + sp) * C;
  if (nch >= 256) {
    for (int ch = t; ch < nch; ch += 256) {
      float a[K], v[K];
      for (int e = 0; e < K; ++e) a[e] = 0.f;
      for (int p = p0; p < p1; ++p) {
        Chunk<T>::unpack(src[(long long)p * nch + ch], v);
#pragma unroll
        for (int e = 0; e < K; ++e) a[e] += v[e];
      }
      for (int e = 0; e < K; ++e) out[ch * K + e] = a[e];
    }
    return;
  }
  const int pg = 256 / nch;
  const int g = t / nch, ch = t % nch;
  float a[K], v[K];
  for (int e = 0; e < K; ++e) a[e] = 0.f;
  if (g < pg) {
    for (int p = p0 + g; p < p1; p += pg) {
      Chunk<T>::unpack(src[(long long)p * nch + ch], v);
#pragma unroll
      for (int e = 0; e < K; ++e) a[e] += v[e];
    }
    for (int e = 0; e < K; ++e) red[(g * nch + ch) * K + e] = a[e];
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    float s = 0.f;
    for (int gg = 0; gg < pg; ++gg) s += red[gg * C + c];
    out[c] = s;
  }
}

// sums[n][c] = sum over the splits of partial[n][split][c]: grid (N, ceil(C/64)), 64 channels x 4 split groups
__global__ void __launch_bounds__(256) gap_reduce_kernel(const float* partial, int splits, int C, float* sums) {
  __shared__ float red[256];
  const int n = blockIdx.x, t = threadIdx.x;
  const int c = blockIdx.y * 64 + (t & 63), sg = t >> 6;
  // eight independent partial sums per thread (eight loads in flight: the depthwise producers write up to 512
  // tile partials per image), combined in a fixed order
  float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const float* base = partial + (long long)n * splits * C + c;
    int sp = sg;
    for (; sp + 28 < splits; sp += 32)
#pragma unroll
      for (int u = 0; u < 8; ++u) a8[u] += base[(long long)(sp + 4 * u) * C];
    for (int u = 0; sp < splits; sp += 4, ++u) a8[u & 7] += base[(long long)sp * C];
  }
  const float a = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
  red[t] = a;
  __syncthreads();
  if (sg == 0 && c < C) sums[(long long)n * C + c] = red[t] + red[t + 64] + red[t + 128] + red[t + 192];
}

// SqueezeExcite MLP from the pooled sums, spread over the chip (one block per image would leave most CUs
// idle at the distillation batch of 4): hidden = act(W1 mean + b1), one wave per hidden unit, grid
// (N, ceil(Cr / 4)); gate = sigmoid(W2 hidden + b2), one wave per channel, grid (N, ceil(C / 4)).  Lanes
// stride the reduction axis (coalesced weight rows), xor-shuffle reduction.
__global__ void __launch_bounds__(256) se_hidden_kernel(const float* sums, int HW, int C, const float* w1,
                                                        const float* b1, int Cr, int act, float beta, float* hid) {
  const int n = blockIdx.x, lane = threadIdx.x & 63;
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (r >= Cr) return;
  const float inv = 1.f / (float)HW;
  const float* m = sums + (long long)n * C;
  const float* wr = w1 + (long long)r * C;
  // four independent partial sums (eight loads in flight per lane: the B7's 2304..3840-channel rows are a 36..60-step
  // dependent chain otherwise), combined in a fixed order
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = lane;
  for (; c + 192 < C; c += 256) {
    s0 += wr[c] * (m[c] * inv);
    s1 += wr[c + 64] * (m[c + 64] * inv);
    s2 += wr[c + 128] * (m[c + 128] * inv);
    s3 += wr[c + 192] * (m[c + 192] * inv);
  }
  for (; c < C; c += 64) s0 += wr[c] * (m[c] * inv);
  float s = (s0 + s1) + (s2 + s3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) hid[(long long)n * Cr + r] = apply_act(s + (b1 ? b1[r] : 0.f), act, beta);
}

__global__ void __launch_bounds__(256) se_out_kernel(const float* hid, int C, int Cr, const float* w2, const float* b2,
                                                     float* gate) {
  const int n = blockIdx.x, lane = threadIdx.x & 63;
  const int c = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float* h = hid + (long long)n * Cr;
  float s = 0.f;
  for (int r = lane; r < Cr; r += 64) s += w2[(long long)c * Cr + r] * h[r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) gate[(long long)n * C + c] = sigmoidf_(s + (b2 ? b2[c] : 0.f));
}

// Two-launch SqueezeExcite from the pool partials (the three launches above -- reduce, hidden, out -- were ~20 us per
// SE block, most of it the hidden kernel's 36..60-step load chain over the B7's long W1 rows and two launch
// boundaries).  Launch 1, grid (N, ceil(C/64)): each block pools its 64 channels (gap_reduce_kernel's order) and
// multiplies them into the Cr hidden units' W1 columns -- one thread per hidden unit, its 64 weights as 16 loads in
// flight -- and writes those Cr partial dot products into the partial rows it alone read (se_hpart_at); launch 2,
// grid (N, ceil(C/256)): every block sums the ceil(C/64) partial products of each hidden unit (fixed order), applies
// b1 + act into LDS, and gives each thread one channel's gate.  Deterministic and batch-independent; the caller
// checks that the hidden partials fit (se2_fits).
__device__ __forceinline__ long long se_hpart_at(int n, int splits, int C, int cb, int r) {
  const int w = C - cb * 64 < 64 ? C - cb * 64 : 64;   // the block's channel width: its partial columns
  return ((long long)n * splits + r / w) * C + cb * 64 + r % w;
}

template <bool V4>
__global__ void __launch_bounds__(256) se_pool_w1_kernel(float* partial, int splits, int HW, int C, const float* w1,
                                                         int Cr) {
  __shared__ float red[256];
  __shared__ __attribute__((aligned(16))) float mloc[64];
  const int n = blockIdx.x, cb = blockIdx.y, t = threadIdx.x;
  const int c = cb * 64 + (t & 63), sg = t >> 6;
  float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const float* base = partial + (long long)n * splits * C + c;
    int sp = sg;
    for (; sp + 28 < splits; sp += 32)
#pragma unroll
      for (int u = 0; u < 8; ++u) a8[u] += base[(long long)(sp + 4 * u) * C];
    for (int u = 0; sp < splits; sp += 4, ++u) a8[u & 7] += base[(long long)sp * C];
  }
  red[t] = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
  __syncthreads();   // every read of this block's partial columns is done: they may take the hidden partials
  if (sg == 0) mloc[t] = c < C ? (red[t] + red[t + 64] + red[t + 128] + red[t + 192]) * (1.f / (float)HW) : 0.f;
  __syncthreads();
  const int w = C - cb * 64 < 64 ? C - cb * 64 : 64;
  for (int r = t; r < Cr; r += 256) {
    const float* wr = w1 + (long long)r * C + cb * 64;
    float s = 0.f;
    if (V4 && w == 64) {
      float4 q[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) q[j] = reinterpret_cast<const float4*>(wr)[j];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        // explicit fused multiply-adds in the scalar path's order: which path runs depends on W1's alignment only,
        // and left to contraction the vectoriser paired these products into packed multiplies (no fusion)
        s = __builtin_fmaf(q[j].x, mloc[4 * j], s);
        s = __builtin_fmaf(q[j].y, mloc[4 * j + 1], s);
        s = __builtin_fmaf(q[j].z, mloc[4 * j + 2], s);
        s = __builtin_fmaf(q[j].w, mloc[4 * j + 3], s);
      }
    } else {
      for (int j = 0; j < w; ++j) s = __builtin_fmaf(wr[j], mloc[j], s);
    }
    partial[se_hpart_at(n, splits, C, cb, r)] = s;
  }
}

template <bool V4>
__global__ void __launch_bounds__(256) se_gate_out_kernel(const float* partial, int splits, int C, const float* b1,
                                                          int Cr, int act, float beta, const float* w2, const float* b2,
                                                          float* gate) {
  // 64 channels per block, four threads per channel, each over a quarter of the channel's W2 row (at most Cr / 4
  // floats, its loads all in flight), combined in a fixed order: 256 channels per block with one thread per row
  // (40 float4 loads each at the B7's Cr = 160, a few in flight at a time) ran 8-15 us per call on 60 blocks
  extern __shared__ __attribute__((aligned(16))) float se_lds[];
  float* hid = se_lds;                        // [Cr]
  float* red = se_lds + ((Cr + 3) & ~3);      // [4][64]
  const int n = blockIdx.x, t = threadIdx.x;
  const int ncb = (C + 63) / 64;
  for (int r = t; r < Cr; r += 256) {
    float s = 0.f;
#pragma unroll 8
    for (int cb = 0; cb < ncb; ++cb) s += partial[se_hpart_at(n, splits, C, cb, r)];
    hid[r] = apply_act(s + (b1 ? b1[r] : 0.f), act, beta);
  }
  __syncthreads();
  const int cl = t & 63, part = t >> 6;
  const int c = blockIdx.y * 64 + cl;
  const int Q = ((Cr + 15) / 16) * 4;   // per-part row span, a multiple of 4 (float4 aligned in every row)
  const int rb = part * Q, re = rb + Q < Cr ? rb + Q : Cr;
  float s = 0.f;
  if (c < C) {
    const float* wr = w2 + (long long)c * Cr;
    if (V4) {
      int r = rb;
      for (; r + 16 <= re; r += 16) {
        float4 q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = *reinterpret_cast<const float4*>(wr + r + 4 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // explicit fused multiply-adds, the scalar path's order
          s = __builtin_fmaf(q[j].x, hid[r + 4 * j], s);
          s = __builtin_fmaf(q[j].y, hid[r + 4 * j + 1], s);
          s = __builtin_fmaf(q[j].z, hid[r + 4 * j + 2], s);
          s = __builtin_fmaf(q[j].w, hid[r + 4 * j + 3], s);
        }
      }
      for (; r < re; ++r) s = __builtin_fmaf(wr[r], hid[r], s);
    } else {
      for (int r = rb; r < re; ++r) s = __builtin_fmaf(wr[r], hid[r], s);
    }
  }
  red[part * 64 + cl] = s;
  __syncthreads();
  if (part == 0 && c < C) {
    const float g = ((red[cl] + red[64 + cl]) + red[128 + cl]) + red[192 + cl];
    gate[(long long)n * C + c] = sigmoidf_(g + (b2 ? b2[c] : 0.f));
  }
}

// the hidden partials of every channel block fit in the partial columns it read: Cr <= splits x (its width)
static bool se2_fits(int splits, int C, int Cr) {
  const int wl = C - ((C + 63) / 64 - 1) * 64;
  return Cr <= (long long)splits * wl && Cr <= 4096;
}

static void se_two_launch(float* partial, int splits, int N, int HW, int C, const float* w1, const float* b1, int Cr,
                          const float* w2, const float* b2, int act, float beta, float* gate, hipStream_t s) {
  const bool v1 = (reinterpret_cast<uintptr_t>(w1) & 15) == 0 && C % 4 == 0;
  const bool v2 = (reinterpret_cast<uintptr_t>(w2) & 15) == 0 && Cr % 4 == 0;
  const dim3 g1(N, (C + 63) / 64), g2(N, (C + 63) / 64);
  if (v1) hipLaunchKernelGGL(se_pool_w1_kernel<true>, g1, dim3(256), 0, s, partial, splits, HW, C, w1, Cr);
  else hipLaunchKernelGGL(se_pool_w1_kernel<false>, g1, dim3(256), 0, s, partial, splits, HW, C, w1, Cr);
  const size_t lds = (size_t)(((Cr + 3) & ~3) + 256) * sizeof(float);
  if (v2) hipLaunchKernelGGL(se_gate_out_kernel<true>, g2, dim3(256), lds, s, partial, splits, C, b1, Cr, act, beta, w2, b2, gate);
  else hipLaunchKernelGGL(se_gate_out_kernel<false>, g2, dim3(256), lds, s, partial, splits, C, b1, Cr, act, beta, w2, b2, gate);
}

static bool se2_enabled() {
  const char* e = getenv("HISEG_SE2");   // 0: the three-launch path (A/B timing, the equivalence test); read per call
  return !(e && atoi(e) == 0);
}

// gate holds the pooled sums on entry and the gate on exit; scratch (>= N * Cr floats) takes the hidden units
static void se_mlp(const float* w1, const float* b1, int Cr, const float* w2, const float* b2, int act, float beta, int N,
                   int HW, int C, float* scratch, float* gate, hipStream_t s) {
  hipLaunchKernelGGL(se_hidden_kernel, dim3(N, (Cr + 3) / 4), dim3(256), 0, s, gate, HW, C, w1, b1, Cr, act, beta, scratch);
  hipLaunchKernelGGL(se_out_kernel, dim3(N, (C + 3) / 4), dim3(256), 0, s, scratch, C, Cr, w2, b2, gate);
}

template <typename T>
__global__ void __launch_bounds__(256) channel_scale_kernel(const void* x, int N, long long HW, int C, const float* gate,
                                                            void* out) {
  constexpr int K = Chunk<T>::N;
  const int nch = C / K;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)N * HW * nch;
  if (gid >= total) return;
  const int ch = (int)(gid % nch);
  const long long n = gid / nch / HW;
  float v[K];
  Chunk<T>::unpack(reinterpret_cast<const uint4*>(x)[gid], v);
  const float* g = gate + n * C + ch * K;
#pragma unroll
  for (int e = 0; e < K; ++e) v[e] *= g[e];
  reinterpret_cast<uint4*>(out)[gid] = Chunk<T>::pack(v);
}

// ------------------------------------------------------------------ depthwise conv + BN + act
// Block = CT channel-chunk lanes x R strip rows (CT = min(C/V, 256); blockIdx.z = chunk group), one image
// (blockIdx.y) and a contiguous range of output strips (blockIdx.x).  A strip is XS consecutive output
// pixels of one row: the (XS-1)*stride + K input columns of each filter row are loaded once and reused by
// the XS outputs, the K weights of a filter row once per strip (cached in L1).  32-bit indices only.
// With gap != nullptr every block also writes the per-channel sum of its outputs (after BN + act) to
// gap[(n * tiles + tile) * C + c] -- the SqueezeExcite global average pool fused into the producer.
constexpr int kDwXS = 4;

template <typename T, int KS, int ST>
__global__ void __launch_bounds__(256) dwconv_kernel(const void* in, int H, int W, int C, const float* w,
                                                     const float* scale, const float* shift, int act, void* out,
                                                     int Ho, int Wo, float* gap) {
  constexpr int V = Chunk<T>::N;
  constexpr int NIN = (kDwXS - 1) * ST + KS;
  __shared__ float red[256 * V];
  const int nch = C / V;
  const int g0 = blockIdx.z * 256;
  const int CT = (nch - g0) < 256 ? (nch - g0) : 256;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int ch = g0 + cl;
  const bool live = r < R;
  const int n = blockIdx.y, tiles = gridDim.x, tile = blockIdx.x;
  const int sx = (Wo + kDwXS - 1) / kDwXS;
  const int strips = Ho * sx;
  const int s0 = (int)((long long)strips * tile / tiles), s1 = (int)((long long)strips * (tile + 1) / tiles);
  const int c = ch * V;
  const int pad = KS / 2;
  float sc[V], sh[V], gs[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { sc[e] = scale[c + e]; sh[e] = shift[c + e]; gs[e] = 0.f; }
  const uint4* src = reinterpret_cast<const uint4*>(in) + (long long)n * H * W * nch;
  uint4* dst = reinterpret_cast<uint4*>(out) + (long long)n * Ho * Wo * nch;
  if (live) {
    for (int st = s0 + r; st < s1; st += R) {
      const int oy = st / sx;
      const int ox0 = (st - oy * sx) * kDwXS;
      float acc[kDwXS][V];
#pragma unroll
      for (int xo = 0; xo < kDwXS; ++xo)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[xo][e] = 0.f;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const int iy = oy * ST - pad + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        float wk[KS][V];
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          const float4* wp = reinterpret_cast<const float4*>(w + (ky * KS + kx) * C + c);
#pragma unroll
          for (int q = 0; q < V / 4; ++q) {
            const float4 f = wp[q];
            wk[kx][4 * q] = f.x; wk[kx][4 * q + 1] = f.y; wk[kx][4 * q + 2] = f.z; wk[kx][4 * q + 3] = f.w;
          }
        }
        const uint4* row = src + (long long)iy * W * nch + ch;
        const int ix0 = ox0 * ST - pad;
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
          const int ix = ix0 + j;
          if ((unsigned)ix >= (unsigned)W) continue;
          float v[V];
          Chunk<T>::unpack(row[(long long)ix * nch], v);
#pragma unroll
          for (int xo = 0; xo < kDwXS; ++xo) {
            const int kx = j - xo * ST;
            if (kx < 0 || kx >= KS) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) acc[xo][e] += wk[kx][e] * v[e];
          }
        }
      }
#pragma unroll
      for (int xo = 0; xo < kDwXS; ++xo) {
        if (ox0 + xo >= Wo) break;
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          o[e] = apply_act(acc[xo][e] * sc[e] + sh[e], act);
          gs[e] += o[e];
        }
        dst[((long long)oy * Wo + ox0 + xo) * nch + ch] = Chunk<T>::pack(o);
      }
    }
  }
  if (gap == nullptr) return;
#pragma unroll
  for (int e = 0; e < V; ++e) red[t * V + e] = gs[e];
  __syncthreads();
  if (r == 0) {
    for (int rr = 1; rr < R; ++rr)
#pragma unroll
      for (int e = 0; e < V; ++e) gs[e] += red[(rr * CT + cl) * V + e];
    float* gp = gap + ((long long)n * tiles + tile) * C + c;
#pragma unroll
    for (int e = 0; e < V; ++e) gp[e] = gs[e];
  }
}

// bf16 depthwise conv, round 2: the kernel above re-reads a thread's K*K x 8 f32 weights (800 B at K = 5) for
// every 4-output strip -- more L1/L2 traffic than the activations themselves on the low-resolution wide layers
// (k5 s1 at 30x40 x 672 channels ran at ~0.5 TB/s).  Here a thread owns 4 channels (8 B of the NHWC row) and
// holds their K*K x 4 weights in registers for all of its strips; a block is CT channel quads x R strip rows
// (CT chosen on the host to fill the 256 threads), and the strip ranges are longer (hiseg_dw_gap_tiles).  Per
// output the arithmetic is the kernel above's: same tap order, same fused multiply-adds, same epilogue.
template <int KS, int ST, bool ZP = false>
__global__ void __launch_bounds__(256) dwconv_q_kernel(const void* in, int H, int W, int C, const float* w,
                                                       const float* scale, const float* shift, int act, void* out,
                                                       int Ho, int Wo, float* gap, int CT, int xcd) {
  constexpr int NIN = (kDwXS - 1) * ST + KS;
  __shared__ float red[256 * 4];
  const int nq = C >> 2;
  // block order as dwconv_t_kernel's (xcd 2: XCD-major, channel groups fastest; 0: launched order)
  int tile = blockIdx.x, n = blockIdx.y, gz = blockIdx.z;
  if (xcd) {
    const int nwg = gridDim.x * gridDim.y * gridDim.z;
    const int orig = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    int wg = xcd_major(orig, nwg);
    if (xcd == 2) {
      gz = wg % gridDim.z;
      wg /= gridDim.z;
      tile = wg % gridDim.x;
      n = wg / gridDim.x;
    } else {
      tile = wg % gridDim.x;
      wg /= gridDim.x;
      n = wg % gridDim.y;
      gz = wg / gridDim.y;
    }
  }
  const int g0 = gz * CT;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int q = g0 + cl < nq ? g0 + cl : nq - 1;   // (a ragged last group's spare lanes redo the last quad)
  const bool live = r < R && g0 + cl < nq;
  const int tiles = gridDim.x;
  const int sx = (Wo + kDwXS - 1) / kDwXS;
  const int strips = Ho * sx;
  const int s0 = (int)((long long)strips * tile / tiles), s1 = (int)((long long)strips * (tile + 1) / tiles);
  const int c = q * 4;
  const int pad = KS / 2;
  float sc[4], sh[4], gs[4], wk[KS * KS][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { sc[e] = scale[c + e]; sh[e] = shift[c + e]; gs[e] = 0.f; }
#pragma unroll
  for (int k = 0; k < KS * KS; ++k) {
    const float4 f = *reinterpret_cast<const float4*>(w + k * C + c);
    wk[k][0] = f.x; wk[k][1] = f.y; wk[k][2] = f.z; wk[k][3] = f.w;
  }
  const uint2* src = reinterpret_cast<const uint2*>(in) + (long long)n * H * W * nq;
  uint2* dst = reinterpret_cast<uint2*>(out) + (long long)n * Ho * Wo * nq;
  if (live) {
    for (int st = s0 + r; st < s1; st += R) {
      const int oy = st / sx;
      const int ox0 = (st - oy * sx) * kDwXS;
      float acc[kDwXS][4];
#pragma unroll
      for (int xo = 0; xo < kDwXS; ++xo)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[xo][e] = 0.f;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const int iy = oy * ST - pad + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        const uint2* row = src + (long long)iy * W * nq + q;
        const int ix0 = ox0 * ST - pad;
        uint2 raw[NIN];
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
          const int ix = ix0 + j;
          raw[j] = (unsigned)ix < (unsigned)W ? row[(long long)ix * nq] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
          const int ix = ix0 + j;
          // ZP: the out-of-image columns were loaded as zeros above and fma(w, 0, acc) == acc in value -- no
          // exec-mask branch per tap (as dwconv_t_kernel's ZP form)
          if (!ZP && (unsigned)ix >= (unsigned)W) continue;
          const float v[4] = {__uint_as_float(raw[j].x << 16), __uint_as_float(raw[j].x & 0xffff0000u),
                              __uint_as_float(raw[j].y << 16), __uint_as_float(raw[j].y & 0xffff0000u)};
#pragma unroll
          for (int xo = 0; xo < kDwXS; ++xo) {
            const int kx = j - xo * ST;
            if (kx < 0 || kx >= KS) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[xo][e] += wk[ky * KS + kx][e] * v[e];
          }
        }
      }
#pragma unroll
      for (int xo = 0; xo < kDwXS; ++xo) {
        if (ox0 + xo >= Wo) break;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = apply_act(acc[xo][e] * sc[e] + sh[e], act);
          gs[e] += o[e];
        }
        dst[((long long)oy * Wo + ox0 + xo) * nq + q] = make_uint2(f2bf2(o[0], o[1]), f2bf2(o[2], o[3]));
      }
    }
  }
  if (gap == nullptr) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) red[t * 4 + e] = gs[e];
  __syncthreads();
  if (r == 0 && live) {
    for (int rr = 1; rr < R; ++rr)
#pragma unroll
      for (int e = 0; e < 4; ++e) gs[e] += red[(rr * CT + cl) * 4 + e];
    float* gp = gap + ((long long)n * tiles + tile) * C + c;
#pragma unroll
    for (int e = 0; e < 4; ++e) gp[e] = gs[e];
  }
}

// LDS-tiled depthwise conv (bf16; round 4).  dwconv_q_kernel gathers every tap straight from global memory (8-B loads,
// each input pixel fetched by up to K x ceil(K / 4) threads through L1 / L2): 0.6 TB/s on the distillation step's
// B7 stages.  Here a block owns an 8 x 16 output tile of one image and 64 channels: the (7 ST + K) x (15 ST + K)
// input window is loaded once into LDS with 16-B loads (a pixel's 64 channels = 128 contiguous bytes, 8 lanes), then
// every thread computes 4-channel x 4-column strips from LDS (8-B reads; pixel stride 136 B to spread the banks).
// Per output the arithmetic is dwconv_q_kernel's exactly -- same taps skipped outside the image, same tap order, same
// fused multiply-adds and epilogue -- so the outputs are bit-identical to it.  SE pool: one partial per (image, tile)
// (hiseg_dw_gap_tiles = ceil(Ho / 8) x ceil(Wo / 16), independent of the batch).
//
// CP (round 6): channels per thread.  CP 4: a thread = one channel quad x 2 strips (16 quads x 16 strip groups per
// block); CP 2: one channel pair x 4 strips (32 pairs x 8 groups).  The k5 form's 25 taps x CP f32 weights live in
// registers: at CP 4 that is 100 VGPRs and the kernel held 256 + 6 AGPRs (one wave per SIMD, one block per CU, the
// window load of the next block never overlapped this one's compute); at CP 2, 50.  Same per-output arithmetic.
constexpr int kDwTH = 8, kDwTW = 16, kDwCG = 64, kDwPS = kDwCG * 2 + 8;
template <int KS, int ST, bool ZP = false, int CP = 4>
__global__ void __launch_bounds__(256) dwconv_t_kernel(const void* in, int H, int W, int C, const float* w,
                                                       const float* scale, const float* shift, int act, void* out,
                                                       int Ho, int Wo, float* gap, int xcd) {
  constexpr int IH = (kDwTH - 1) * ST + KS, IW = (kDwTW - 1) * ST + KS;
  constexpr int NIN = (kDwXS - 1) * ST + KS;
  constexpr int NSTRIP = kDwTH * (kDwTW / kDwXS);   // 32 strips of 4 outputs per channel quad
  extern __shared__ __attribute__((aligned(16))) char dws[];
  const int t = threadIdx.x;
  // block -> (tile, image, channel group): grid (tiles, N, groups) as launched, or (xcd != 0) the XCD-major
  // bijective remap of the linear block id -- the dispatcher deals consecutive blocks round-robin to the 8 XCDs, so
  // launched order puts a tile's neighbours (which re-read its halo rows / columns) and the other channel groups of
  // its pixels (a 64-channel group is 128 B at a pixel stride of 2C bytes: it straddles cache lines it shares with
  // the next group) behind other L2s; remapped, each XCD works through a contiguous run of (group, tile) blocks.
  // Same per-tile arithmetic: outputs bit-identical in every order.
  int bt = blockIdx.x, n = blockIdx.y, gz = blockIdx.z;
  if (xcd) {
    const int nwg = gridDim.x * gridDim.y * gridDim.z;
    const int orig = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    int wg = xcd_major(orig, nwg);
    if (xcd == 2) {   // channel groups fastest: the groups of one tile share the cache lines a group straddles
      gz = wg % gridDim.z;
      wg /= gridDim.z;
      bt = wg % gridDim.x;
      n = wg / gridDim.x;
    } else {
      bt = wg % gridDim.x;
      wg /= gridDim.x;
      n = wg % gridDim.y;
      gz = wg / gridDim.y;
    }
  }
  const int g0 = gz * kDwCG;
  const int ntx = (Wo + kDwTW - 1) / kDwTW;
  const int ty = bt / ntx, tx = bt - ty * ntx;
  const int oy0 = ty * kDwTH, ox0 = tx * kDwTW;
  const int iy0 = oy0 * ST - KS / 2, ix0 = ox0 * ST - KS / 2;
  const int nch = C >> 3;   // 8-channel chunks
  // ---- input window -> LDS: 8 chunks (128 B) per pixel, zeros outside the image / past C
  // batches of 8 loads per thread in flight before their LDS writes (a load -> wait -> write loop left every block
  // waiting out ~8 global latencies one after another)
  const uint4* src = reinterpret_cast<const uint4*>(in) + (long long)n * H * W * nch;
  constexpr int NLD = (IH * IW * 8 + 255) / 256;
#pragma unroll
  for (int b0 = 0; b0 < NLD; b0 += 8) {
    uint4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = t + 256 * (b0 + u);
      const int pix = idx >> 3, ck = idx & 7;
      const int hy = pix / IW, hx = pix - hy * IW;
      const int iy = iy0 + hy, ix = ix0 + hx, ch = (g0 >> 3) + ck;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (b0 + u < NLD && idx < IH * IW * 8 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W && ch < nch)
        v[u] = src[((long long)iy * W + ix) * nch + ch];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = t + 256 * (b0 + u);
      if (b0 + u < NLD && idx < IH * IW * 8)
        *reinterpret_cast<uint4*>(dws + (idx >> 3) * kDwPS + (idx & 7) * 16) = v[u];
    }
  }
  // ---- compute: thread = channel group qd of CP channels (64 / CP per block) x strips it, it + NG, ... (NG groups)
  static_assert(CP == 2 || CP == 4, "CP: 2 or 4 channels per thread");
  constexpr int NQ = kDwCG / CP, NG = 256 / NQ, NP = CP / 2;
  const int qd = t % NQ, it = t / NQ;
  const int c = g0 + qd * CP;
  const bool live = c < C;
  const int cc = live ? c : 0;
  typedef float f2v __attribute__((ext_vector_type(2)));
  float wk[ZP ? 1 : KS * KS][CP], sc[CP], sh[CP], gs[CP];
  f2v wp[ZP ? KS * KS : 1][NP];   // ZP: the weights as channel pairs (packed-FMA operands)
#pragma unroll
  for (int k = 0; k < KS * KS; ++k) {
    float f[CP];
    if constexpr (CP == 4) {
      const float4 q = *reinterpret_cast<const float4*>(w + k * C + cc);
      f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
    } else {
      const float2 q = *reinterpret_cast<const float2*>(w + k * C + cc);
      f[0] = q.x; f[1] = q.y;
    }
#pragma unroll
    for (int e = 0; e < CP; ++e) {
      if constexpr (ZP) wp[k][e >> 1][e & 1] = f[e];
      else wk[k][e] = f[e];
    }
  }
#pragma unroll
  for (int e = 0; e < CP; ++e) { sc[e] = scale[cc + e]; sh[e] = shift[cc + e]; gs[e] = 0.f; }
  // held in registers for every strip (the compiler otherwise re-loads each tap's weights at its use)
#pragma unroll
  for (int k = 0; k < KS * KS; ++k) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if constexpr (ZP) asm volatile("" : "+v"(wp[k][p]));
      else asm volatile("" : "+v"(wk[k][2 * p]), "+v"(wk[k][2 * p + 1]));
    }
  }
  __syncthreads();
  const int nq = C / CP;
  // one uint per channel pair of the output (bf16 x 2)
  unsigned* dst = reinterpret_cast<unsigned*>(out) + (long long)n * Ho * Wo * (C >> 1);
#pragma unroll
  for (int sj = 0; sj < NSTRIP / NG; ++sj) {
    const int st = it + NG * sj;
    const int ry = st / (kDwTW / kDwXS), rx = (st - ry * (kDwTW / kDwXS)) * kDwXS;
    const int oy = oy0 + ry, ox = ox0 + rx;
    if (!live || oy >= Ho) continue;
    float acc[kDwXS][CP];
#pragma unroll
    for (int xo = 0; xo < kDwXS; ++xo)
#pragma unroll
      for (int e = 0; e < CP; ++e) acc[xo][e] = 0.f;
    if constexpr (ZP) {
      // no per-tap bounds test -- the window holds zeros outside the image, and fma(w, 0, acc) == acc in value (the
      // sign of an all-zero sum may differ from skipping the tap): straight-line packed FMAs, no exec-mask branches.
      // Per element the same fma(w, v, acc) chain in the same tap order as below.
      f2v a2[kDwXS][NP];
#pragma unroll
      for (int xo = 0; xo < kDwXS; ++xo)
#pragma unroll
        for (int p = 0; p < NP; ++p) a2[xo][p] = f2v{0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const char* row = dws + ((ry * ST + ky) * IW + rx * ST) * kDwPS + qd * 2 * CP;
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
          unsigned raw[NP];
          if constexpr (CP == 4) {
            const uint2 r2 = *reinterpret_cast<const uint2*>(row + j * kDwPS);
            raw[0] = r2.x; raw[NP - 1] = r2.y;
          } else {
            raw[0] = *reinterpret_cast<const unsigned*>(row + j * kDwPS);
          }
          f2v v[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p) v[p] = f2v{__uint_as_float(raw[p] << 16), __uint_as_float(raw[p] & 0xffff0000u)};
#pragma unroll
          for (int xo = 0; xo < kDwXS; ++xo) {
            const int kx = j - xo * ST;
            if (kx < 0 || kx >= KS) continue;
#pragma unroll
            for (int p = 0; p < NP; ++p) a2[xo][p] = __builtin_elementwise_fma(wp[ky * KS + kx][p], v[p], a2[xo][p]);
          }
        }
        // k5 at CP 4: one window row's reads live at a time (hoisting all 5 rows' reads took 251-256 VGPRs)
        if constexpr (KS == 5 && CP == 4) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int xo = 0; xo < kDwXS; ++xo)
#pragma unroll
        for (int e = 0; e < CP; ++e) acc[xo][e] = a2[xo][e >> 1][e & 1];
    }
#pragma unroll
    for (int ky = 0; ky < (ZP ? 0 : KS); ++ky) {
      const int iy = oy * ST - KS / 2 + ky;
      if ((unsigned)iy >= (unsigned)H) continue;
      const char* row = dws + ((ry * ST + ky) * IW + rx * ST) * kDwPS + qd * 2 * CP;
#pragma unroll
      for (int j = 0; j < NIN; ++j) {
        const int ix = ox * ST - KS / 2 + j;
        if ((unsigned)ix >= (unsigned)W) continue;
        unsigned raw[NP];
        if constexpr (CP == 4) {
          const uint2 r2 = *reinterpret_cast<const uint2*>(row + j * kDwPS);
          raw[0] = r2.x; raw[NP - 1] = r2.y;
        } else {
          raw[0] = *reinterpret_cast<const unsigned*>(row + j * kDwPS);
        }
        float v[CP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          v[2 * p] = __uint_as_float(raw[p] << 16);
          v[2 * p + 1] = __uint_as_float(raw[p] & 0xffff0000u);
        }
#pragma unroll
        for (int xo = 0; xo < kDwXS; ++xo) {
          const int kx = j - xo * ST;
          if (kx < 0 || kx >= KS) continue;
#pragma unroll
          for (int e = 0; e < CP; ++e) acc[xo][e] += wk[ZP ? 0 : ky * KS + kx][e] * v[e];
        }
      }
    }
#pragma unroll
    for (int xo = 0; xo < kDwXS; ++xo) {
      if (ox + xo >= Wo) break;
      float o[CP];
#pragma unroll
      for (int e = 0; e < CP; ++e) {
        o[e] = apply_act(acc[xo][e] * sc[e] + sh[e], act);
        gs[e] += o[e];
      }
      unsigned* d = dst + ((long long)oy * Wo + ox + xo) * (C >> 1) + (c >> 1);
      if constexpr (CP == 4) *reinterpret_cast<uint2*>(d) = make_uint2(f2bf2(o[0], o[1]), f2bf2(o[2], o[3]));
      else *d = f2bf2(o[0], o[1]);
    }
  }
  (void)nq;
  if (gap == nullptr) return;
  __syncthreads();   // the window is no longer read: its LDS takes the NG x 64 pool partials
  float* red = reinterpret_cast<float*>(dws);
#pragma unroll
  for (int e = 0; e < CP; ++e) red[t * CP + e] = gs[e];
  __syncthreads();
  if (it == 0 && live) {
    for (int r = 1; r < NG; ++r)
#pragma unroll
      for (int e = 0; e < CP; ++e) gs[e] += red[(r * NQ + qd) * CP + e];
    float* gp = gap + ((long long)n * gridDim.x + bt) * C + c;
#pragma unroll
    for (int e = 0; e < CP; ++e) gp[e] = gs[e];
  }
}

// channel quads per block for dwconv_q_kernel: the fewest z groups whose blocks keep >= 90 % of the 256 threads
// busy (else the best fill seen)
static int dw_quads_per_block(int nq) {
  int best = nq < 256 ? nq : 256, best_fill = 0;
  for (int d = 1; d <= 16; ++d) {
    const int ct = (nq + d - 1) / d;
    if (ct > 256) continue;
    const int fill = (256 / ct) * ct;
    if (fill > best_fill) { best = ct; best_fill = fill; }
    if (fill >= 230) return ct;
  }
  return best;
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

static int chunk_of(int dtype) { return dtype == HISEG_BF16 ? 8 : 4; }

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
  hipLaunchKernelGGL(attn_map_kernel, dim3(nblocks(P, 256)), dim3(256), 0, s, stats, N, H, W, w7, k, att);
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
  hipLaunchKernelGGL(attn_map_kernel, dim3(nblocks(P, 256)), dim3(256), 0, s, stats, N, H, W, w7, k, att);
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

extern "C" int hiseg_gap_splits(int HW) {
  // >= 32 pixels per split (was 512: the B0 student's SE pools over 4 x 20 x 20 ran as 4 blocks, one 400-pixel
  // dependent load chain per thread, 52 us)
  int s = HW / 32;
  if (s < 1) s = 1;
  if (s > 64) s = 64;
  return s;
}

extern "C" int hiseg_se_gate_fwd(int dtype, const void* x, int N, int HW, int C, const float* w1, const float* b1, int Cr,
                                 const float* w2, const float* b2, int act, float act_beta, float* partial, float* gate,
                                 hiseg_stream_t stream) {
  HISEG_REQUIRE(x && w1 && w2 && partial && gate && N > 0 && HW > 0 && C > 0 && Cr > 0, HISEG_ERR_BAD_ARG,
                "se_gate: bad args");
  const int K = chunk_of(dtype);
  HISEG_REQUIRE(C % K == 0, HISEG_ERR_BAD_SHAPE, "se_gate: C must be chunk aligned");
  const int nch = C / K;
  const int splits = hiseg_gap_splits(HW);
  HISEG_REQUIRE((long long)splits * C >= Cr, HISEG_ERR_BAD_SHAPE, "se_gate: partial buffer below N * Cr");
  const size_t lds = nch >= 256 ? 0 : (size_t)(256 / nch) * C * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  DISPATCH_T(dtype, gap_partial_kernel, dim3(N, splits), dim3(256), lds, s, x, HW, C, splits, partial);
  if (se2_enabled() && se2_fits(splits, C, Cr)) {
    se_two_launch(partial, splits, N, HW, C, w1, b1, Cr, w2, b2, act, act_beta, gate, s);
    return hiseg_check_launch("se_gate");
  }
  // the pooled sums go through the gate buffer: each se_gate block reads its image's row into LDS before
  // it overwrites that row with the gate
  hipLaunchKernelGGL(gap_reduce_kernel, dim3(N, (C + 63) / 64), dim3(256), 0, s, partial, splits, C, gate);
  se_mlp(w1, b1, Cr, w2, b2, act, act_beta, N, HW, C, partial, gate, s);   // partial (consumed): hidden units
  return hiseg_check_launch("se_gate");
}

extern "C" int hiseg_channel_scale_fwd(int dtype, const void* x, int N, int HW, int C, const float* gate, void* out,
                                       hiseg_stream_t stream) {
  // C > 0: C = 0 passed the chunk test and reached a zero-block launch
  HISEG_REQUIRE(x && gate && out && N > 0 && HW > 0 && C > 0 && C % chunk_of(dtype) == 0, HISEG_ERR_BAD_ARG,
                "channel_scale: bad args");
  const long long total = (long long)N * HW * (C / chunk_of(dtype));
  DISPATCH_T(dtype, channel_scale_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, x, N, (long long)HW,
             C, gate, out);
  return hiseg_check_launch("channel_scale");
}

extern "C" int hiseg_dw_gap_tiles(int N, int Ho, int Wo) {
  // strip ranges of >= 2 strips, at most 2048 / N per image.  (Ranges of >= 16 strips, which amortised a thread's
  // register-held weights, left the deep low-resolution layers with ~120 blocks: the B7's k5 2304-channel
  // depthwise conv over 4 x 20 x 20 ran at 0.3 TB/s, tools/train_layer_profile.py --leg distill.)
  const int strips = Ho * ((Wo + kDwXS - 1) / kDwXS);
  int t = 2048 / (N > 0 ? N : 1);
  if (t < 1) t = 1;
  int by_len = strips / 2;
  if (by_len < 1) by_len = 1;
  return t < by_len ? t : by_len;
}

// Which depthwise kernel takes a layer: the LDS-tiled one for bf16 layers of 192..2047 channels, stride 1 or k5.
// HISEG_DWCONV_Q=0: the round-2 v5 bf16 kernel (8 channels per thread, weights re-read per strip), A/B only.  It
// also turns the tiles off, so hiseg_dw_gap_parts (the SE-pool partial count callers size buffers by) and
// dwconv_launch always agree on the kernel.
static bool dw_q_enabled() {
  const char* e = getenv("HISEG_DWCONV_Q");
  return !(e && atoi(e) == 0);
}

static bool dw_use_tiles(int dtype, int C, int K, int stride) {
  // HISEG_DWCONV_T: 0 never, 2 every bf16 layer (A/B timing, the bit-identity test); read per call
  const char* e = getenv("HISEG_DWCONV_T");
  const int m = e ? atoi(e) : 1;
  if (dtype != HISEG_BF16 || m == 0 || !dw_q_enabled()) return false;
  // tools/dw_bench.py (profiles/r4_dw_bench.txt; round 5 with the XCD-major order, profiles/r5_dwconv_xcd.txt): the
  // tiles win on the 64..1344-channel stride-1 layers and the >= 192-channel k5 stride-2 ones; the gather kernel on
  // the 32-channel layers, the k3 stride-2 ones, the 144-channel k5 stride-2 one and the 20 x 20 x >= 2304-channel ones
  return m == 2 || (C < 2048 && ((stride == 1 && C >= 64) || (K == 5 && C >= 192)));
}

extern "C" int hiseg_dw_gap_parts(int dtype, int N, int Ho, int Wo, int C, int K, int stride) {
  // SE-pool partials per image of this layer: one per 8 x 16 output tile for the LDS-tiled kernel (independent of
  // the batch), else hiseg_dw_gap_tiles' strip ranges
  if (dw_use_tiles(dtype, C, K, stride)) return ((Ho + kDwTH - 1) / kDwTH) * ((Wo + kDwTW - 1) / kDwTW);
  return hiseg_dw_gap_tiles(N, Ho, Wo);
}

static size_t dw_lds(int KS, int ST) {
  const size_t win = (size_t)((kDwTH - 1) * ST + KS) * ((kDwTW - 1) * ST + KS) * kDwPS;
  return win > 256 * 4 * sizeof(float) ? win : 256 * 4 * sizeof(float);
}

// block order of the LDS-tiled kernel (HISEG_DWCONV_XCD, read per call): 2 (default) XCD-major, channel groups
// fastest; 1 XCD-major, tiles fastest; 0 launched order.  Round 5 (profiles/r5_dwconv_xcd.txt): HBM bytes per launch
// 309 -> 208 -> 149 MB on the C2 k5 layer (147 MB algorithmic), time equal or better on every layer shape.
static int dw_xcd_remap() {
  const char* e = getenv("HISEG_DWCONV_XCD");
  return e ? atoi(e) : 2;
}

// the gather kernel without its per-tap column test (HISEG_DWCONV_QZP=0: with it everywhere; read per call, A/B).
// Round 5 (profiles/r5_dwconv_xcd.txt): 2-10 % faster on the k3 and k5 stride-2 layers; the k5 stride-1 form drops to
// 2 waves per SIMD (176 VGPRs) and runs 10-33 % slower, so it keeps the test
static bool dw_zero_pad_q(int K, int stride) {
  const char* e = getenv("HISEG_DWCONV_QZP");
  return !(e && e[0] == '0') && (K == 3 || stride == 2);
}

// the same for the gather kernel (HISEG_DWCONV_QXCD, read per call; profiles/r5_dwconv_xcd.txt: order 2 cuts its HBM
// bytes up to 3.2x -- k5 s1 C2 layer 267 -> 83 MB -- and is 1-13 % faster on all but one layer shape, +1 % there)
static int dw_xcd_remap_q() {
  const char* e = getenv("HISEG_DWCONV_QXCD");
  return e ? atoi(e) : 2;
}

// the stride-2 windows exceed the default 64 KiB of dynamic LDS (k5: 19 x 35 pixels = 90 KiB)
template <int KS, int ST>
static void dw_t_attr() {
  static bool done = false;
  if (!done) {
    (void)hipFuncSetAttribute((const void*)dwconv_t_kernel<KS, ST, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dw_lds(KS, ST));
    (void)hipFuncSetAttribute((const void*)dwconv_t_kernel<KS, ST, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dw_lds(KS, ST));
    (void)hipFuncSetAttribute((const void*)dwconv_t_kernel<KS, ST, false, 2>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)dw_lds(KS, ST));
    (void)hipFuncSetAttribute((const void*)dwconv_t_kernel<KS, ST, true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dw_lds(KS, ST));
    done = true;
  }
}

// the LDS-tiled kernel without per-tap bounds tests (HISEG_DWCONV_ZP, read per call: 2 (default) every layer, 1 the
// k3 layers only, 0 none).  Round 5 (profiles/r5_dwconv_xcd.txt): k3 1-18 % faster, k5 20-31 % (its form holds 248-256
// VGPRs, 1-2 waves per SIMD, and is still faster than the 3-wave form with the branches)
static bool dw_zero_pad(int K) {
  const char* e = getenv("HISEG_DWCONV_ZP");
  const int m = e ? atoi(e) : 2;
  return m == 2 || (K == 3 && m == 1);
}

// channels per thread of the LDS-tiled kernel (HISEG_DWCONV_CP, read per call: 4 or 2 everywhere; default: 2 on the
// k5 layers, whose CP-4 form holds 256 VGPRs + AGPRs, and on the k3 layers of < 512 channels).  tools/dw_bench.py,
// profiles/r6_dw_cp.txt: k5 stride 1 1.7-2.1x faster (B7 480 ch @80x80 53.0 -> 30.0 us, 1344 @40x40 37.6 -> 21.7, C2
// 240 @60x80 142 -> 69, 1152 @15x20 64.5 -> 32.8), k3 stride 1 3-7 % faster up to 288 channels, 6 % slower at 960
static int dw_cp(int K, int C) {
  const char* e = getenv("HISEG_DWCONV_CP");
  const int m = e ? atoi(e) : 0;
  return m == 2 || m == 4 ? m : (K == 5 || C < 512 ? 2 : 4);
}

static int dwconv_launch(int dtype, const void* in, int N, int H, int W, int C, int K, int stride, const float* w,
                         const float* scale, const float* shift, int act, void* out, int Ho, int Wo, float* gap,
                         hipStream_t s) {
  HISEG_REQUIRE(in && w && scale && shift && out && N > 0 && H > 0 && W > 0, HISEG_ERR_BAD_ARG, "dwconv: bad args");
  HISEG_REQUIRE(act != HISEG_ACT_SWISH, HISEG_ERR_BAD_ARG, "dwconv: Swish(beta) is not an EfficientNet activation");
  HISEG_REQUIRE(C % chunk_of(dtype) == 0, HISEG_ERR_BAD_SHAPE, "dwconv: C must be chunk aligned");
  HISEG_REQUIRE((K == 3 || K == 5) && (stride == 1 || stride == 2), HISEG_ERR_BAD_SHAPE, "dwconv: K %d stride %d", K,
                stride);
  HISEG_REQUIRE(Ho == (H + 2 * (K / 2) - K) / stride + 1 && Wo == (W + 2 * (K / 2) - K) / stride + 1, HISEG_ERR_BAD_SHAPE,
                "dwconv: output grid mismatch");
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(w) & 15) == 0 && (long long)H * W * C < (1ll << 31), HISEG_ERR_BAD_SHAPE,
                "dwconv: weights must be 16-B aligned, image < 2^31 elements");
  const int nch = C / chunk_of(dtype);
  const int nq = C / 4, ctq = dw_quads_per_block(nq);
  const int tiles = hiseg_dw_gap_tiles(N, Ho, Wo);
  dim3 grid(tiles, N, (nch + 255) / 256);
  dim3 gridq(tiles, N, (nq + ctq - 1) / ctq);
  const bool dwq = dw_q_enabled();
  const bool dwt = dw_use_tiles(dtype, C, K, stride);
  const int tiles2 = ((Ho + kDwTH - 1) / kDwTH) * ((Wo + kDwTW - 1) / kDwTW);
  const dim3 gridt(tiles2, N, (C + kDwCG - 1) / kDwCG);
#define DW_L(KS, ST)                                                                                          \
  do {                                                                                                        \
    if (dtype == HISEG_BF16 && dwt) {                                                                         \
      dw_t_attr<KS, ST>();                                                                                    \
      const bool zp = dw_zero_pad(KS), cp2 = dw_cp(KS, C) == 2;                                                    \
      if (zp && cp2)                                                                                          \
        hipLaunchKernelGGL((dwconv_t_kernel<KS, ST, true, 2>), gridt, dim3(256), dw_lds(KS, ST), s, in, H, W, \
                           C, w, scale, shift, act, out, Ho, Wo, gap, dw_xcd_remap());                        \
      else if (zp)                                                                                            \
        hipLaunchKernelGGL((dwconv_t_kernel<KS, ST, true>), gridt, dim3(256), dw_lds(KS, ST), s, in, H, W, C, \
                           w, scale, shift, act, out, Ho, Wo, gap, dw_xcd_remap());                           \
      else if (cp2)                                                                                           \
        hipLaunchKernelGGL((dwconv_t_kernel<KS, ST, false, 2>), gridt, dim3(256), dw_lds(KS, ST), s, in, H,   \
                           W, C, w, scale, shift, act, out, Ho, Wo, gap, dw_xcd_remap());                     \
      else                                                                                                    \
        hipLaunchKernelGGL((dwconv_t_kernel<KS, ST, false>), gridt, dim3(256), dw_lds(KS, ST), s, in, H, W,   \
                           C, w, scale, shift, act, out, Ho, Wo, gap, dw_xcd_remap());                        \
    }                                                                                                         \
    else if (dtype == HISEG_BF16 && dwq)                                                                      \
    {                                                                                                         \
      if (dw_zero_pad_q(KS, ST))                                                                              \
        hipLaunchKernelGGL((dwconv_q_kernel<KS, ST, true>), gridq, dim3(256), 0, s, in, H, W, C, w, scale,    \
                           shift, act, out, Ho, Wo, gap, ctq, dw_xcd_remap_q());                              \
      else                                                                                                    \
        hipLaunchKernelGGL((dwconv_q_kernel<KS, ST, false>), gridq, dim3(256), 0, s, in, H, W, C, w, scale,   \
                           shift, act, out, Ho, Wo, gap, ctq, dw_xcd_remap_q());                              \
    }                                                                                                         \
    else if (dtype != HISEG_BF16)                                                                             \
      hipLaunchKernelGGL((dwconv_kernel<float, KS, ST>), grid, dim3(256), 0, s, in, H, W, C, w, scale, shift,  \
                         act, out, Ho, Wo, gap);                                                              \
    else                                                                                                      \
      hipLaunchKernelGGL((dwconv_kernel<bf16_t, KS, ST>), grid, dim3(256), 0, s, in, H, W, C, w, scale, shift, \
                         act, out, Ho, Wo, gap);                                                              \
  } while (0)
  if (K == 3 && stride == 1) DW_L(3, 1);
  else if (K == 3) DW_L(3, 2);
  else if (stride == 1) DW_L(5, 1);
  else DW_L(5, 2);
#undef DW_L
  return hiseg_check_launch("dwconv");
}

extern "C" int hiseg_dwconv_fwd(int dtype, const void* in, int N, int H, int W, int C, int K, int stride, const float* w,
                                const float* scale, const float* shift, int act, void* out, int Ho, int Wo,
                                hiseg_stream_t stream) {
  return dwconv_launch(dtype, in, N, H, W, C, K, stride, w, scale, shift, act, out, Ho, Wo, nullptr,
                       (hipStream_t)stream);
}

extern "C" int hiseg_dwconv_gap_fwd(int dtype, const void* in, int N, int H, int W, int C, int K, int stride,
                                    const float* w, const float* scale, const float* shift, int act, void* out, int Ho,
                                    int Wo, float* gap_partial, hiseg_stream_t stream) {
  HISEG_REQUIRE(gap_partial, HISEG_ERR_BAD_ARG, "dwconv_gap: null partial buffer");
  return dwconv_launch(dtype, in, N, H, W, C, K, stride, w, scale, shift, act, out, Ho, Wo, gap_partial,
                       (hipStream_t)stream);
}

extern "C" int hiseg_se_gate_partials_fwd(float* partial, int splits, int N, int HW, int C, const float* w1,
                                          const float* b1, int Cr, const float* w2, const float* b2, int act, float* gate,
                                          hiseg_stream_t stream) {
  HISEG_REQUIRE(partial && w1 && w2 && gate && splits > 0 && N > 0 && HW > 0 && C > 0 && Cr > 0, HISEG_ERR_BAD_ARG,
                "se_gate_partials: bad args");
  hipStream_t s = (hipStream_t)stream;
  HISEG_REQUIRE(act != HISEG_ACT_SWISH, HISEG_ERR_BAD_ARG, "se_gate_partials: Swish(beta) is not an EfficientNet act");
  if (se2_enabled() && se2_fits(splits, C, Cr)) {
    se_two_launch(partial, splits, N, HW, C, w1, b1, Cr, w2, b2, act, 1.f, gate, s);
    return hiseg_check_launch("se_gate_partials");
  }
  // pooled sums through the gate buffer (read into LDS per image before the gate overwrites them)
  HISEG_REQUIRE((long long)splits * C >= Cr, HISEG_ERR_BAD_SHAPE, "se_gate_partials: partial buffer below N * Cr");
  hipLaunchKernelGGL(gap_reduce_kernel, dim3(N, (C + 63) / 64), dim3(256), 0, s, partial, splits, C, gate);
  se_mlp(w1, b1, Cr, w2, b2, act, 1.f, N, HW, C, partial, gate, s);   // partial (consumed) holds the hidden units
  return hiseg_check_launch("se_gate_partials");
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
