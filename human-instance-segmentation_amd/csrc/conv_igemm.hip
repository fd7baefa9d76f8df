// Implicit-GEMM convolution on CDNA4 MFMA (gfx950).
//
// GEMM view (see include/hiseg.h, hiseg_conv2d_fwd):   D[co][px] = sum_k W[co][k] * X[px][k]
//   rows of the MFMA "A" operand  = output channels (weights, K-contiguous, packed by the host)
//   cols of the MFMA "B" operand  = output pixels   (gathered on the fly from NHWC activations)
// With this orientation every lane ends up holding 4 consecutive output channels of one
// pixel (16x16 accumulator map: col = lane&15, row = 4*(lane>>4)+r), which is what the
// channel-contiguous NHWC epilogue stores.
//
// bf16: v_mfma_f32_16x16x32_bf16 (8 k-values per lane per fragment = one 16-B chunk).
// f32 : v_mfma_f32_16x16x4_f32 (exact f32, parity mode); a 16-B chunk holds 4 k-values and
//       is consumed by 4 MFMAs (the k order inside a chunk is permuted identically for both
//       operands, so the contraction is unchanged).
//
// Tiling: one workgroup = 256 threads = 4 waves, output tile BCO x BPX, K block = 8 chunks
// (64 bf16 / 32 f32).  Both operand tiles are staged through LDS as 128-B rows of 8 chunks,
// chunk c of row r stored at slot c ^ ((r>>1)&7): conflict-free for the ds_read_b128 lane
// groups of the fragment reads (MI355X_MICROARCH.md §LDS) and for the row-wise stores.
// Two LDS stages; the next K block is gathered into registers while the current one feeds
// the MFMAs (register-staged double buffering, one barrier per K block).
//
// This file is the generic kernel alone: conv_dispatch.cpp decides when it runs (conv_generic_launch, splitk_plan).
#include <cstdlib>
#include "conv_common.h"

namespace hiseg {

// SPLIT: split-K (grid.z = splits, a.kper K blocks each) for small grids with long K loops -- the SE-gated
// EfficientNet projections at the deep stages (B7: 2304 -> 384 over 4 x 20 x 20 pixels = 39 tiles of 128 x 128
// for 36 K blocks: one global round trip per K block on one workgroup per CU).  Each split stores its raw f32
// tile to the caller's workspace [split][M][Cout_pad]; conv_splitk_reduce_kernel sums the splits in order and
// applies the epilogue (deterministic; within f32 re-association of the unsplit kernel).
// LIN (bf16; 1x1, pad 0, one source, no upsampling; the launcher checks every tensor fits one 2^31-byte buffer
// resource): a chunk's source pixel and channel never change along the K loop except by whole K blocks, so its
// activation, gate and weight byte offsets are computed once and each K block's loads are buffer loads at those
// offsets + a wave-uniform (SGPR) K-block offset -- the per-block 64-bit (n, y, x) -> address products and bounds
// checks were most of the gather's VALU work, the SE-gated layers' more.  Rows outside the GEMM and chunks past
// Cin load zeros through out-of-range offsets; the same values land in LDS as in the general gather.
// LIN 2 (bf16; any KH x KW <= 32 taps and stride, ungated, one un-upsampled source): each thread stages one chunk
// column, so its (tap, channel) is per thread -- per K block one byte delta ((ky Ws + kx) Cstride + ci) 2 is added
// to each row's tap-(0, 0) offset, and a per-row tap mask (bit ky KW + kx: the tap lies inside the image) replaces
// the bounds checks.
template <typename T, typename TO, int BCO, int BPX, int WCO, int WPX, bool SPLIT = false, int LIN = 0>
__global__ void __launch_bounds__(256) conv_igemm_kernel(ConvArgs a) {
  constexpr int KCH = Chunk<T>::N;
  constexpr int BK = 8 * KCH;
  constexpr int TM = BCO / (WCO * 16);
  constexpr int TN = BPX / (WPX * 16);
  constexpr int A_CH = (BPX * 8 + 255) / 256;
  constexpr int W_CH = (BCO * 8 + 255) / 256;
  constexpr int STAGE = (BCO + BPX) * 8;  // uint4 slots per stage
  constexpr bool A_FULL = (BPX * 8) % 256 == 0;  // every thread owns A_CH act chunks
  constexpr bool W_FULL = (BCO * 8) % 256 == 0;
  static_assert(WCO * WPX == 4, "4 waves");
  static_assert(TM >= 1 && TN >= 1, "tile");

  extern __shared__ __attribute__((aligned(16))) uint4 smem[];

  const hiseg_conv2d_desc& d = a.d;
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int wco = wave / WPX;
  const int wpx = wave % WPX;
  const int px0 = blockIdx.x * BPX;
  const int co0 = blockIdx.y * BCO;
  const int c = t & 7;  // the chunk this thread stages, every row, every K block

  // ---- per-row pixel decode for the activation gather ----
  int rn[A_CH], riy[A_CH], rix[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int r = (t >> 3) + 32 * i;
    const int m = px0 + r;
    if ((A_FULL || r < BPX) && m < a.M) {
      const int ox = m % d.Wo;
      const int tt = m / d.Wo;
      const int oy = tt % d.Ho;
      rn[i] = tt / d.Ho;
      riy[i] = oy * d.stride - d.pad;
      rix[i] = ox * d.stride - d.pad;
    } else {
      rn[i] = -1; riy[i] = 0; rix[i] = 0;
    }
  }
  // K range of this workgroup (split-K: blocks [kb0, kb1))
  const int kb0 = SPLIT ? (int)blockIdx.z * a.kper : 0;
  const int kb1 = SPLIT ? (kb0 + a.kper < a.nK ? kb0 + a.kper : a.nK) : a.nK;
  // K state of this thread's chunk: k = kb*BK + c*KCH  ->  (ky, kx, ci)
  int ci, ky, kx;
  {
    const int k = kb0 * BK + c * KCH;
    const int tap = k / a.Cin;
    ci = k - tap * a.Cin;
    ky = tap / d.KW;
    kx = tap - ky * d.KW;
  }
  const int Cin = a.Cin;
  const int KW = d.KW;
  static_assert(!LIN || sizeof(T) == 2, "LIN: bf16");
  unsigned voff_a[LIN ? A_CH : 1], voff_g[LIN ? A_CH : 1], voff_w[LIN ? W_CH : 1];
  __amdgpu_buffer_rsrc_t rsA, rsG, rsW;
  if constexpr (LIN == 2) {
    rsA = buf_rsrc(d.srcA, 0x7fffffff);
    rsW = buf_rsrc(d.weight, 0x7fffffff);
    const int ci0 = kb0 * BK + c * KCH;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {   // voff_a: tap-(0, 0) byte offset (wrapping); voff_g: the row's tap mask
      unsigned msk = 0u;
      if (rn[i] >= 0) {
        for (int ky2 = 0; ky2 < d.KH; ++ky2)
          for (int kx2 = 0; kx2 < d.KW; ++kx2) {
            const int iy = riy[i] + ky2, ix = rix[i] + kx2;
            if (iy >= 0 && iy < d.H && ix >= 0 && ix < d.W) msk |= 1u << (ky2 * d.KW + kx2);
          }
      }
      voff_g[i] = msk;
      voff_a[i] = (unsigned)(((rn[i] * a.Hs + riy[i]) * a.Ws + rix[i]) * d.a_cstride + d.a_coff) * 2u;
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      const int r = (t >> 3) + 32 * i;
      voff_w[i] = co0 + r < d.Cout_pad ? (unsigned)(((co0 + r) * d.K_pad + ci0) * 2) : kOobOffset;
    }
  }
  if constexpr (LIN == 1) {
    rsA = buf_rsrc(d.srcA, 0x7fffffff);
    rsG = buf_rsrc(d.in_scale ? d.in_scale : reinterpret_cast<const float*>(d.srcA), 0x7fffffff);
    rsW = buf_rsrc(d.weight, 0x7fffffff);
    const int ci0 = kb0 * BK + c * KCH;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const bool ok = rn[i] >= 0 && riy[i] >= 0 && riy[i] < d.H && rix[i] >= 0 && rix[i] < d.W;
      voff_a[i] = ok ? (unsigned)((((rn[i] * a.Hs + riy[i]) * a.Ws + rix[i]) * d.a_cstride + d.a_coff + ci0) * 2) : kOobOffset;
      voff_g[i] = ok ? (unsigned)((rn[i] * d.Ca + ci0) * 4) : kOobOffset;
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      const int r = (t >> 3) + 32 * i;
      voff_w[i] = co0 + r < d.Cout_pad ? (unsigned)(((co0 + r) * d.K_pad + ci0) * 2) : kOobOffset;
    }
  }

  uint4 ra[A_CH], rw[W_CH];
#pragma unroll
  for (int i = 0; i < W_CH; ++i) rw[i] = make_uint4(0u, 0u, 0u, 0u);

  // SE gate (in_scale) of the gathered chunks: loaded beside the activations, applied when the chunk is stored to
  // LDS (after the current K block's MFMAs), so the loads' latency overlaps the MFMAs instead of stalling the
  // gather -- the gate multiply once made every K block of the deep EfficientNet projections wait for its loads
  // (1.5 us of 3.2 us per block, tools/splitk_bench.py with HISEG_SPLITK sweeps)
  constexpr int GREG = sizeof(T) == 2 ? 2 : 1;   // float4 gate vectors per chunk
  float4 rg[A_CH][GREG];
  bool rgs[A_CH];
  auto gather = [&](int kb) __attribute__((always_inline)) {
    if constexpr (LIN == 2) {
      const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)((kb - kb0) * BK * 2));
      const bool kvalid = ky < d.KH;
      const int tap = ky * KW + kx;
      const unsigned delta = (unsigned)((ky * a.Ws + kx) * d.a_cstride + ci) * 2u;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const bool ok = kvalid && ((voff_g[i] >> tap) & 1u);
        ra[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsA, ok ? voff_a[i] + delta : kOobOffset, 0u, 0));
        rgs[i] = false;
      }
#pragma unroll
      for (int i = 0; i < W_CH; ++i) {
        const int r = (t >> 3) + 32 * i;
        if (W_FULL || r < BCO) rw[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsW, voff_w[i], so, 0));
      }
      return;
    }
    if constexpr (LIN == 1) {
      const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)((kb - kb0) * BK * 2));
      const bool kc = kb * BK + c * KCH < Cin;   // chunks past Cin (the last K block's padding) are zeros
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const unsigned va = kc ? voff_a[i] : kOobOffset;
        ra[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsA, va, so, 0));
        rgs[i] = false;
        if (d.in_scale) {
          rgs[i] = kc && voff_a[i] != kOobOffset;
          const unsigned vg = rgs[i] ? voff_g[i] : kOobOffset;
#pragma unroll
          for (int e = 0; e < GREG; ++e)
            rg[i][e] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsG, vg + 16u * e, 2u * so, 0));
        }
      }
#pragma unroll
      for (int i = 0; i < W_CH; ++i) {
        const int r = (t >> 3) + 32 * i;
        if (W_FULL || r < BCO) rw[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsW, voff_w[i], so, 0));
      }
      return;
    }
    const bool kvalid = ky < d.KH;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      rgs[i] = false;
      if (rn[i] >= 0 && kvalid) {
        const int iy = riy[i] + ky, ix = rix[i] + kx;
        if (iy >= 0 && iy < d.H && ix >= 0 && ix < d.W) {
          if (ci < d.Ca) {
            const int sy = d.a_up == 2 ? (iy >> 1) : iy;
            const int sx = d.a_up == 2 ? (ix >> 1) : ix;
            const long long off = (((long long)rn[i] * a.Hs + sy) * a.Ws + sx) * d.a_cstride + d.a_coff + ci;
            v = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(d.srcA) + off);
            if (d.in_scale) {
              const float* s = d.in_scale + (long long)rn[i] * d.Ca + ci;
              rgs[i] = true;
              if (a.ins_vec) {   // 16-B aligned gate rows: vector loads
#pragma unroll
                for (int e = 0; e < GREG; ++e) rg[i][e] = *reinterpret_cast<const float4*>(s + 4 * e);
              } else {
#pragma unroll
                for (int e = 0; e < GREG; ++e) rg[i][e] = make_float4(s[4 * e], s[4 * e + 1], s[4 * e + 2], s[4 * e + 3]);
              }
            }
          } else {
            const long long off = (((long long)rn[i] * d.H + iy) * d.W + ix) * d.b_cstride + d.b_coff + (ci - d.Ca);
            v = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(d.srcB) + off);
          }
        }
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      const int r = (t >> 3) + 32 * i;
      if (W_FULL || r < BCO) {
        // the last Cout tile may overhang Cout_pad: clamp the row, zero the value
        const int row = co0 + r < d.Cout_pad ? co0 + r : d.Cout_pad - 1;
        const long long off = (long long)row * d.K_pad + (long long)kb * BK + c * KCH;
        const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(d.weight) + off);
        rw[i] = co0 + r < d.Cout_pad ? v : make_uint4(0u, 0u, 0u, 0u);
      }
    }
  };
  auto advance = [&]() __attribute__((always_inline)) {
    ci += BK;
    while (ci >= Cin) {
      ci -= Cin;
      if (++kx == KW) { kx = 0; ++ky; }
    }
  };
  auto stage_store = [&](int s) __attribute__((always_inline)) {
    uint4* sm = smem + s * STAGE;
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      const int r = (t >> 3) + 32 * i;
      if (W_FULL || r < BCO) sm[swz(r, c)] = rw[i];
    }
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int r = (t >> 3) + 32 * i;
      uint4 v = ra[i];
      if (d.in_scale && rgs[i]) {   // the loader's rounding: bf16(x * gate) (f32: exact product)
        float f[KCH];
        Chunk<T>::unpack(v, f);
#pragma unroll
        for (int e = 0; e < GREG; ++e) {
          f[4 * e] *= rg[i][e].x; f[4 * e + 1] *= rg[i][e].y; f[4 * e + 2] *= rg[i][e].z; f[4 * e + 3] *= rg[i][e].w;
        }
        v = Chunk<T>::pack(f);
      }
      if (A_FULL || r < BPX) sm[BCO * 8 + swz(r, c)] = v;
    }
  };

  floatx4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  gather(kb0);
  stage_store(0);
  __syncthreads();

  for (int kb = kb0; kb < kb1; ++kb) {
    const int cur = (kb - kb0) & 1;
    if (kb + 1 < kb1) {
      advance();
      gather(kb + 1);
    }
    const uint4* sW = smem + cur * STAGE;
    const uint4* sX = sW + BCO * 8;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int ch = s * 4 + (lane >> 4);
      uint4 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = sW[swz(wco * TM * 16 + i * 16 + (lane & 15), ch)];
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[j] = sX[swz(wpx * TN * 16 + j * 16 + (lane & 15), ch)];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (sizeof(T) == 2) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, bfr[j]),
                acc[i][j], 0, 0, 0);
          } else {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[i].x), __uint_as_float(bfr[j].x), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[i].y), __uint_as_float(bfr[j].y), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[i].z), __uint_as_float(bfr[j].z), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[i].w), __uint_as_float(bfr[j].w), acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    if (kb + 1 < kb1) stage_store(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue ----
  int epx[TN], eco[TM];
#pragma unroll
  for (int j = 0; j < TN; ++j) epx[j] = px0 + wpx * TN * 16 + j * 16 + (lane & 15);
#pragma unroll
  for (int i = 0; i < TM; ++i) eco[i] = co0 + wco * TM * 16 + i * 16 + (lane >> 4) * 4;
  if constexpr (SPLIT) {
    float* ws = a.ws + (long long)blockIdx.z * a.M * d.Cout_pad;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        if (epx[j] < a.M && eco[i] < d.Cout_pad)
          *reinterpret_cast<floatx4*>(ws + (long long)epx[j] * d.Cout_pad + eco[i]) = acc[i][j];
    return;
  }
  if (TileEpi<T, TO, TM, TN>::ok(d)) {
    TileEpi<T, TO, TM, TN> ep;
    ep.prefetch(d, a.M, epx, eco);
    ep.store(d, a.M, epx, eco, acc);
  } else {
#pragma clang loop unroll(full)
    for (int i = 0; i < TM; ++i) {
#pragma clang loop unroll(full)
      for (int j = 0; j < TN; ++j) {
        if (epx[j] < a.M) conv_epilogue<T, TO>(a, epx[j], eco[i], acc[i][j]);
      }
    }
  }
}

// Split-K reduction: one thread per (pixel, 4-column quad); the splits are summed in order 0..S-1, then the
// conv epilogue (scale / shift, residual, activation, mul, dual store) of the unsplit kernel.
template <typename T, typename TO>
__global__ void __launch_bounds__(256) conv_splitk_reduce_kernel(ConvArgs a, int splits) {
  const hiseg_conv2d_desc& d = a.d;
  const int nq = d.Cout_pad >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.M * nq) return;
  const int px = (int)(i / nq), co = (int)(i - (long long)px * nq) * 4;
  const long long plane = (long long)a.M * d.Cout_pad;
  const float* p = a.ws + (long long)px * d.Cout_pad + co;
  floatx4 acc = *reinterpret_cast<const floatx4*>(p);
  for (int z = 1; z < splits; ++z) acc += *reinterpret_cast<const floatx4*>(p + z * plane);
  conv_epilogue<T, TO>(a, px, co, acc);
}

// The LIN gather applies (bf16 checked by the caller): 1x1, pad 0, one un-upsampled source, gate rows 16-B aligned,
// every tensor within one buffer resource.  HISEG_IGEMM_LIN=0 keeps the general gather (A/B timing and the
// equivalence test; read per call).
static int lin_ok(const ConvArgs& a) {
  const hiseg_conv2d_desc& d = a.d;
  const char* e = getenv("HISEG_IGEMM_LIN");
  const int mode = e ? atoi(e) : 2;   // 0: general gather, 1: 1x1 only, 2: 1x1 and the tap form
  if (mode == 0) return 0;
  if (d.Cb != 0 || d.a_up != 1 || d.convT) return 0;
  const long long lim = 0x7fff0000ll;
  if ((long long)d.N * a.Hs * a.Ws * d.a_cstride * 2 >= lim) return 0;
  if ((long long)d.Cout_pad * d.K_pad * 2 >= lim) return 0;
  if (d.KH == 1 && d.KW == 1 && d.pad == 0) {
    if (d.in_scale && !a.ins_vec) return 0;
    if (d.in_scale && (long long)d.N * d.Ca * 4 >= lim) return 0;
    return 1;
  }
  if (mode < 2 || d.in_scale || d.KH * d.KW > 32 || a.Cin % 8) return 0;
  return 2;
}

template <typename T, typename TO, int BCO, int BPX, int WCO, int WPX>
static int launch_cfg(const ConvArgs& a, hipStream_t s, int splits) {
  dim3 grid((a.M + BPX - 1) / BPX, (a.d.Cout_pad + BCO - 1) / BCO, splits > 1 ? splits : 1);
  const size_t lds = 2u * (BCO + BPX) * 8u * 16u;
  if constexpr (sizeof(T) == 2) {
    const int lin = lin_ok(a);
    if (lin) {
      if (splits > 1) {
        if (lin == 1) hipLaunchKernelGGL((conv_igemm_kernel<T, TO, BCO, BPX, WCO, WPX, true, 1>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((conv_igemm_kernel<T, TO, BCO, BPX, WCO, WPX, true, 2>), grid, dim3(256), lds, s, a);
        const int r = hiseg_check_launch("conv_igemm_splitk");
        if (r) return r;
        const long long n = (long long)a.M * (a.d.Cout_pad >> 2);
        hipLaunchKernelGGL((conv_splitk_reduce_kernel<T, TO>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, splits);
        return hiseg_check_launch("conv_splitk_reduce");
      }
      if (lin == 1) hipLaunchKernelGGL((conv_igemm_kernel<T, TO, BCO, BPX, WCO, WPX, false, 1>), grid, dim3(256), lds, s, a);
      else hipLaunchKernelGGL((conv_igemm_kernel<T, TO, BCO, BPX, WCO, WPX, false, 2>), grid, dim3(256), lds, s, a);
      return hiseg_check_launch("conv_igemm");
    }
  }
  if (splits > 1) {
    hipLaunchKernelGGL((conv_igemm_kernel<T, TO, BCO, BPX, WCO, WPX, true>), grid, dim3(256), lds, s, a);
    const int r = hiseg_check_launch("conv_igemm_splitk");
    if (r) return r;
    const long long n = (long long)a.M * (a.d.Cout_pad >> 2);
    hipLaunchKernelGGL((conv_splitk_reduce_kernel<T, TO>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, splits);
    return hiseg_check_launch("conv_splitk_reduce");
  }
  hipLaunchKernelGGL((conv_igemm_kernel<T, TO, BCO, BPX, WCO, WPX>), grid, dim3(256), lds, s, a);
  return hiseg_check_launch("conv_igemm");
}

// Tile choice: the widest Cout tile whose overhang past Cout_pad adds <= 1/6 to the MFMA work.
static int igemm_bco(int cp) {
  auto fits = [&](int bco) { return ((cp + bco - 1) / bco) * bco * 6 <= cp * 7; };
  auto padded = [&](int bco) { return ((cp + bco - 1) / bco) * bco; };
  if (cp >= 96 && fits(128)) return 128;
  if (cp >= 48 && fits(64)) return 64;
  // >= 48 columns that fit neither: the 64 / 128 tile with the less overhang (tie: 128), not the narrow 32 / 16 x
  // 256 tiles -- one or four MFMAs per wave per k-step ran the B1 EnhancedUNet's 72- and 144-channel 3x3 layers
  // at 53-80 TFLOP/s (tools: bench.py call_profile top_layers, C3)
  if (cp >= 48) return padded(64) < padded(128) ? 64 : 128;
  if (fits(32)) return 32;
  return 16;
}

// split-K tiles: 128 x 128, or 64 x 128 -- never the narrow 32 / 16 x 256 tiles, whose eight gathered chunks per
// thread made a gated split workgroup several times slower (960 -> 160 over 4 x 40 x 40: 57 us)
static int splitk_bco(int cp) { return cp >= 96 && igemm_bco(cp) == 128 ? 128 : 64; }

// *bco: the Cout tile of the launch (what hiseg_conv2d_last_path reports for the generic kernel)
template <typename T, typename TO>
static int launch_typed(const ConvArgs& a, hipStream_t s, int splits, int* bco) {
  // SE-gated layers as the split-K ones: the narrow 16 / 32 x 256 tiles gather their gated A chunks through
  // registers (the B7's 480 -> 80 projections over 4 x 80 x 80 at 16 x 256 tiles: 66 us per launch)
  static const bool gated_wide = [] { const char* e = getenv("HISEG_GATED_WIDE"); return !(e && atoi(e) == 0); }();
  int tile;
  if (splits > 1 || (gated_wide && a.d.in_scale != nullptr)) {
    tile = splitk_bco(a.d.Cout_pad);
  } else {
    const char* eb = getenv("HISEG_IGEMM_BCO");   // A/B timing: force the Cout tile (read per call)
    tile = eb ? atoi(eb) : igemm_bco(a.d.Cout_pad);
    if (tile != 128 && tile != 64 && tile != 32) tile = 16;
  }
  *bco = tile;
  switch (tile) {
    case 128: return launch_cfg<T, TO, 128, 128, 2, 2>(a, s, splits);
    case 64: return launch_cfg<T, TO, 64, 128, 2, 2>(a, s, splits);
    case 32: return launch_cfg<T, TO, 32, 256, 1, 4>(a, s, splits);
    default: return launch_cfg<T, TO, 16, 256, 1, 4>(a, s, splits);
  }
}

int conv_generic_launch(const ConvArgs& a, hipStream_t s, int splits, int* bco) {
  const bool obf = a.d.out_dtype == HISEG_BF16;
  if (a.d.dtype == HISEG_BF16)
    return obf ? launch_typed<bf16_t, bf16_t>(a, s, splits, bco) : launch_typed<bf16_t, float>(a, s, splits, bco);
  return obf ? launch_typed<float, bf16_t>(a, s, splits, bco) : launch_typed<float, float>(a, s, splits, bco);
}

// Split-K plan of the generic kernel for a bf16 1x1 layer with a long K loop over a small image: splits (>= 2) or 1
// (no split).  The plan depends on the layer and the per-image grid only, never on the batch: an output element's
// f32 summation order (K blocks within a split, then the splits in order) is then the same whether its image is
// computed alone or in a batch, which keeps the exported masks batch-invariant bit for bit
// (test_c2_shape_bf16_properties_and_oracle).  Images of <= 1600 pixels (the EfficientNet's stride-16 / 32
// stages at 640 x 640 and 480 x 640), >= 6 K blocks: nK / 4 splits, 2..8.  The workspace it needs: splits x M x
// Cout_pad f32.
int splitk_plan(const ConvArgs& a) {
  const hiseg_conv2d_desc& d = a.d;
  if (d.dtype != HISEG_BF16 || d.convT || a.nK < 6) return 1;
  // 3x3 layers over images of <= 256 pixels with long K (the B7 EnhancedUNet's 768-channel 3x3 pair over 8 x 16 x 12:
  // the halo kernel gets one 16 x 16 tile per image x 6 Cout tiles = 48 workgroups, 118 TFLOP/s): nK / 4 splits,
  // 2..8, on the generic kernel -- when the caller passes the workspace (the train engine does for <= 8192 pixels in
  // all; a large batch of such images fills the GPU on the halo kernel)
  if (d.KH == 3 && d.KW == 3 && d.stride == 1 && d.a_up == 1 && (long long)d.Ho * d.Wo <= 256 && a.nK >= 24 &&
      d.in_scale == nullptr) {
    int sp = a.nK / 4;
    return sp > 8 ? 8 : sp;
  }
  if (d.KH != 1 || d.KW != 1) return 1;
  // ungated layers take the LDS-DMA ring kernel (conv_fast.hip), which keeps more K blocks in flight: only long
  // K loops split there (the 384 -> 2304 expansion over 4 x 20 x 20 pixels: 17 us unsplit, 31 us split in two)
  if (d.in_scale == nullptr && a.nK < 24) return 1;
  // HISEG_SPLITK=S forces S splits on every layer the split applies to (A/B timing only)
  static const int forced = [] { const char* e = getenv("HISEG_SPLITK"); return e ? atoi(e) : 0; }();
  if (forced > 0) return forced < a.nK ? forced : a.nK;
  if ((long long)d.Ho * d.Wo > 1600) return 1;
  int sp = a.nK / 4;
  if (sp > 8) sp = 8;
  return sp >= 2 ? sp : 2;
}

long long splitk_bytes(const ConvArgs& a, int splits) {
  return splits > 1 ? (long long)splits * a.M * a.d.Cout_pad * 4 : 0;
}

}  // namespace hiseg
