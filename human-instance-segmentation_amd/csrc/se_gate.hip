// SqueezeExcite of the EfficientNet encoder: the global average pool's partials and reduction, the gate MLP from the
// pooled sums (two- and three-launch forms), and the channel scale that applies the gate.
#include "common.h"

namespace hiseg {

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

}  // namespace hiseg

using namespace hiseg;

#define DISPATCH_T(dtype, KERNEL, ...)                                                        \
  do {                                                                                        \
    if ((dtype) == HISEG_BF16) hipLaunchKernelGGL(KERNEL<bf16_t>, __VA_ARGS__);               \
    else if ((dtype) == HISEG_F32) hipLaunchKernelGGL(KERNEL<float>, __VA_ARGS__);            \
    else { hiseg_set_error("unsupported dtype %d", (int)(dtype)); return HISEG_ERR_BAD_DTYPE; } \
  } while (0)

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
