// The EfficientNet encoder's forward depthwise convs (+ folded BN + act, + the fused SqueezeExcite pool partials):
// three kernels, the HISEG_DWCONV_* knobs, and the one plan (DwPlan) that says which kernel takes a layer.
#include "common.h"
#include "gfx950_prims.h"

namespace hiseg {

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

}  // namespace hiseg

using namespace hiseg;

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
// also turns the tiles off (the tests and tools/dw_bench.py use it to mean "the round-2 kernel"); read per call.
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

// One layer's launch, decided in one place.  Whoever needs to know which kernel will run, or how many SE-pool partial
// rows per image it writes, asks dw_plan: hiseg_dw_gap_parts (what callers size the partial buffer by) returns
// `parts`, dwconv_launch launches exactly this plan.  Every kernel writes one partial row per blockIdx.x, so parts is
// grid.x by construction.  Built per call (every knob above is read per call); not cached.  Takes the output grid,
// which is all hiseg_dw_gap_parts is given -- nothing here depends on H or W beyond it.
enum DwKernel { kDwF32, kDwBf16x8, kDwQuad, kDwTile };   // dwconv_kernel<float>, <bf16_t>, dwconv_q_kernel, dwconv_t_kernel

struct DwPlan {
  DwKernel kernel;
  bool zp;      // quad, tile: the form without per-tap bounds tests
  int cp;       // tile: channels per thread, 2 or 4
  int xcd;      // quad, tile: block order
  int ctq;      // quad: channel quads per block
  dim3 grid;
  size_t lds;   // dynamic LDS bytes
  int parts;    // SE-pool partial rows per image
};

static DwPlan dw_plan(int dtype, int N, int Ho, int Wo, int C, int K, int stride) {
  DwPlan p = {kDwF32, false, 0, 0, 0, dim3(), 0, 0};
  if (dw_use_tiles(dtype, C, K, stride)) {
    // one partial per 8 x 16 output tile, independent of the batch
    p.kernel = kDwTile;
    p.zp = dw_zero_pad(K);
    p.cp = dw_cp(K, C);
    p.xcd = dw_xcd_remap();
    p.grid = dim3(((Ho + kDwTH - 1) / kDwTH) * ((Wo + kDwTW - 1) / kDwTW), N, (C + kDwCG - 1) / kDwCG);
    p.lds = dw_lds(K, stride);
  } else if (dtype == HISEG_BF16 && dw_q_enabled()) {
    const int nq = C / 4;
    p.kernel = kDwQuad;
    p.zp = dw_zero_pad_q(K, stride);
    p.xcd = dw_xcd_remap_q();
    p.ctq = nq > 0 ? dw_quads_per_block(nq) : 1;   // (C < 4 is never launched; hiseg_dw_gap_parts validates nothing)
    p.grid = dim3(hiseg_dw_gap_tiles(N, Ho, Wo), N, (nq + p.ctq - 1) / p.ctq);
  } else {
    p.kernel = dtype == HISEG_BF16 ? kDwBf16x8 : kDwF32;
    p.grid = dim3(hiseg_dw_gap_tiles(N, Ho, Wo), N, (C / chunk_of(dtype) + 255) / 256);
  }
  p.parts = (int)p.grid.x;
  return p;
}

extern "C" int hiseg_dw_gap_parts(int dtype, int N, int Ho, int Wo, int C, int K, int stride) {
  return dw_plan(dtype, N, Ho, Wo, C, K, stride).parts;
}

// launches plan p for one (K, stride); a: the arguments every depthwise kernel takes, in ... gap
template <int KS, int ST, typename... A>
static void dw_launch_plan(const DwPlan& p, hipStream_t s, A... a) {
  auto go = [&](auto kernel, auto... tail) { hipLaunchKernelGGL(kernel, p.grid, dim3(256), p.lds, s, a..., tail...); };
  switch (p.kernel) {
    case kDwTile:
      dw_t_attr<KS, ST>();
      if (p.zp && p.cp == 2) go(dwconv_t_kernel<KS, ST, true, 2>, p.xcd);
      else if (p.zp) go(dwconv_t_kernel<KS, ST, true>, p.xcd);
      else if (p.cp == 2) go(dwconv_t_kernel<KS, ST, false, 2>, p.xcd);
      else go(dwconv_t_kernel<KS, ST, false>, p.xcd);
      break;
    case kDwQuad:
      if (p.zp) go(dwconv_q_kernel<KS, ST, true>, p.ctq, p.xcd);
      else go(dwconv_q_kernel<KS, ST, false>, p.ctq, p.xcd);
      break;
    case kDwBf16x8: go(dwconv_kernel<bf16_t, KS, ST>); break;
    case kDwF32: go(dwconv_kernel<float, KS, ST>); break;
  }
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
  const DwPlan p = dw_plan(dtype, N, Ho, Wo, C, K, stride);
  if (K == 3 && stride == 1) dw_launch_plan<3, 1>(p, s, in, H, W, C, w, scale, shift, act, out, Ho, Wo, gap);
  else if (K == 3) dw_launch_plan<3, 2>(p, s, in, H, W, C, w, scale, shift, act, out, Ho, Wo, gap);
  else if (stride == 1) dw_launch_plan<5, 1>(p, s, in, H, W, C, w, scale, shift, act, out, Ho, Wo, gap);
  else dw_launch_plan<5, 2>(p, s, in, H, W, C, w, scale, shift, act, out, Ho, Wo, gap);
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
