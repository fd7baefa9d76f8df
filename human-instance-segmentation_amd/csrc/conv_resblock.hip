// A whole 64-channel ResidualBlock in one launch (gfx950, bf16, eval mode; refinement.py:31-55 / unet.py:35-58):
//   y = act2(bn2(conv2(act1(bn1(conv1(x))))) + x),   both convs 3x3 / stride 1 / pad 1, 64 -> 64.
//
// The two-launch path (conv_hwc variant 107 twice) writes the intermediate h to HBM and reads it back, and reads x a
// second time as the residual.  Here a workgroup (four waves) owns a 16 x 16 output tile of one image and keeps h on
// the CU:
//   1. x over the tile plus a 2-pixel halo (20 x 20 pixels, all 64 channels) arrives by LDS-DMA; out-of-image lanes
//      carry an offset past num_records and read zeros.
//   2. conv1 over the tile plus a 1-pixel ring (18 x 18), scale / shift / activation in f32, rounded to bf16 with
//      f2bf2 -- the bits conv1's launch stores today -- and written to LDS over the (dead) input; ring pixels outside
//      the image are written as zeros: they are conv2's zero padding, not conv1 evaluated outside the image.
//   3. conv2 from that LDS tile; conv_hwc's epilogue (residual tile by LDS-DMA, conversion in place, 16-B stores).
//
// Layout.  Input and intermediate share one pixel pitch of 20: input pixel q = hy * 20 + hx is image pixel
// (y0 - 2 + hy, x0 - 2 + hx), ring pixel m = iy * 20 + ix is image pixel (y0 - 1 + iy, x0 - 1 + ix), so conv1's tap
// (ky, kx) of ring pixel m reads input pixel m + 20 ky + kx and conv2's tap of output (oy, ox) reads ring pixel
// (oy + ky) * 20 + ox + kx: a tap is a constant shift of a linear index.  conv1 therefore runs over 23 fragments of
// 16 consecutive linear ring pixels (368 >= 18 * 20; the columns ix = 18, 19 are computed and dropped: 23 / 16 = 1.44
// x conv1's MFMAs, 1.22 x the pair's), conv2 over the 16 output rows.  A 32-channel slice of a pixel is 64 B, one
// plane per slice; 16-B chunk c of pixel p sits at slot c ^ 2 ((p >> 2) & 1), which keeps the ds_read_b128 of 16
// consecutive pixels conflict-free at every shift (conv_hwc's swizzle on the linear index: 20 is a multiple of 4).
//
// Waves: w = 2 ph + wc; wc = the 32-Cout group (= the slice of the intermediate the wave writes), ph = the pixel
// half: conv1 fragments 12 ph .. 12 ph + 11 (fragment 23 does not exist: the wave repeats 22 and drops the copy),
// conv2 output rows 8 ph .. 8 ph + 7.
//
// Per output element the accumulation order is conv_hwc's: slices in order; within a slice kx-major, ky inner; one
// v_mfma_f32_16x16x32_bf16 per (slice, tap); the same epilogue expressions -- so the block equals the two launches bit
// for bit.  Weights (hiseg.ops.frag_pack order) are streamed one (slice, kx) block ahead, conv2's first block during
// conv1's last.
//
// LDS: two input planes of 416 pixels (26 DMA pieces; the last fragment's taps reach pixel 409) = 53248 B; the
// intermediate (2 x 368 pixels = 47104 B) and the epilogue tile (256 rows x 128 B = 32768 B) overlay it behind
// barriers.  Three workgroups fit a CU's 160 KiB; the register budget is set for two.
#include "conv_common.h"

namespace hiseg {

constexpr int RB_HP = 20;                 // pixel pitch of the input halo and the intermediate
constexpr int RB_NPI = 26;                // DMA pieces (16 pixels x 64 B) per input plane
constexpr int RB_PLANE_I = RB_NPI * 1024;   // bytes of an input plane
constexpr int RB_NF = 23;                 // conv1 fragments (16 linear ring pixels each)
constexpr int RB_PLANE_M = RB_NF * 1024;    // bytes of an intermediate plane
constexpr int RB_LDS = 2 * RB_PLANE_I;

template <int ACT1, int ACT2>
__global__ void __launch_bounds__(256, 2) conv_resblock_kernel(hiseg_conv2d_desc d1, hiseg_conv2d_desc d2) {
  constexpr int NW = 4, FPW = 12, NR2 = 8;
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wc = w & 1, ph = w >> 1;

  // ---- XCD-major bijective remap (conv_hwc's): the tiles of one image stay on one XCD's L2
  const int ntx = (d1.W + 15) >> 4, nty = (d1.H + 15) >> 4;
  int tl = xcd_major(blockIdx.x, gridDim.x);
  const int tx = tl % ntx;
  tl /= ntx;
  const int ty = tl % nty;
  const int n = tl / nty;
  const int y0 = ty * 16, x0 = tx * 16;
  const int H = d1.H, W = d1.W;

  const __amdgpu_buffer_rsrc_t rF1 = buf_rsrc(d1.weight_frag, 64 * 9 * 64 * 2);
  const __amdgpu_buffer_rsrc_t rF2 = buf_rsrc(d2.weight_frag, 64 * 9 * 64 * 2);
  const __amdgpu_buffer_rsrc_t rA = buf_rsrc(d1.srcA, d1.N * H * W * d1.a_cstride * 2);

  // ---- A fragments (hiseg.ops.frag_pack, one 64-channel block): (16-row Cout tile ct, slice sl, tap) at
  // (((ct * 9 + tap) * 2 + sl) * 64 + lane) * 16 B; the wave's two tiles are 2 wc, 2 wc + 1
  auto load_blk = [&](u32x4 (&af)[3][2], const __amdgpu_buffer_rsrc_t& rF, int sl, int kx) __attribute__((always_inline)) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const unsigned a_lane = (unsigned)(2 * wc) * 18u * 1024u + (unsigned)ln * 16u;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const unsigned so = __builtin_amdgcn_readfirstlane(((unsigned)(ky * 3 + kx) * 2u + (unsigned)sl) * 1024u);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        af[ky][i] = __builtin_amdgcn_raw_buffer_load_b128(rF, a_lane + (unsigned)i * 18u * 1024u, so, 0);
    }
  };

  const unsigned lds_base = (unsigned)(uintptr_t)(lds_void*)smem;
  const char* lds_c = reinterpret_cast<const char*>(smem);
  char* lds_w = reinterpret_cast<char*>(smem);

  // ---- prologue: both input planes (52 pieces of 1 KiB, 13 per wave), the weights of conv1's block (slice 0, kx 0).
  // Piece g = plane g / 26, pixels 16 (g % 26) + lane / 4; the lane's LDS slot is lane % 4, so it fetches chunk
  // (lane % 4) ^ swz(pixel).
#pragma unroll
  for (int k = 0; k < 13; ++k) {
    const int g = w + NW * k;
    const int sl = g >= RB_NPI ? 1 : 0, pc = g - RB_NPI * sl;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int p = 16 * pc + (ln >> 2);
    const int hy = p / RB_HP, hx = p - RB_HP * hy;
    const int iy = y0 - 2 + hy, ix = x0 - 2 + hx;
    const bool ok = hy < RB_HP && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    const int chunk = (ln & 3) ^ halo_row_swz(p);
    const unsigned off =
        ok ? (unsigned)((((n * H + iy) * W + ix) * d1.a_cstride + d1.a_coff + 32 * sl + chunk * 8) * 2) : kOobOffset;
    lds_dma16(rA, lds_base + (unsigned)(RB_PLANE_I * sl + 1024 * pc), off);
  }
  u32x4 af[3][2], an[3][2];
  load_blk(af, rF1, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int j16 = lane & 15, c4 = lane >> 4;

  // ================================================================================================ conv1
  floatx4 acc[2][FPW];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int k = 0; k < FPW; ++k) acc[i][k] = floatx4{0.f, 0.f, 0.f, 0.f};
  // fragment k of this wave = ring pixels 16 (12 ph + k) .. + 15; the last one of ph 1 repeats fragment 22
  const int klast = ph ? FPW - 2 : FPW - 1;
  {
    constexpr int RA = 4;   // B fragments read ahead of their MFMAs
    auto block1 = [&](int sl, auto kxc, bool last) __attribute__((always_inline)) {
      constexpr int KX = decltype(kxc)::value;
      if (!last) load_blk(an, rF1, KX < 2 ? sl : sl + 1, KX < 2 ? KX + 1 : 0);
      else load_blk(an, rF2, 0, 0);
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int j = ln & 15, cc = ln >> 4;
      // B fragment (ky, k): input pixels 16 (12 ph + k) + 20 ky + KX + j, channels 8 cc .. + 7 of slice sl; the slot
      // swizzle depends on (j + 20 ky + KX) alone (16 k and 192 ph are multiples of 8)
      int adr[3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int tt = j + RB_HP * ky + KX;
        adr[ky] = RB_PLANE_I * sl + (16 * FPW * ph + tt) * 64 + ((cc ^ halo_row_swz(tt)) << 4);
      }
      auto rd = [&](int idx) __attribute__((always_inline)) -> u32x4 {
        const int ky = idx / FPW, k = idx % FPW;
        const int ko = k == FPW - 1 ? klast * 1024 : k * 1024;
        return *reinterpret_cast<const u32x4*>(lds_c + adr[ky] + ko);
      };
      u32x4 bq[RA + 1];
#pragma unroll
      for (int r = 0; r < RA; ++r) bq[r] = rd(r);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int idx = 0; idx < 3 * FPW; ++idx) {
        if (idx + RA < 3 * FPW) bq[(idx + RA) % (RA + 1)] = rd(idx + RA);
        __builtin_amdgcn_sched_barrier(0);
        const int ky = idx / FPW, k = idx % FPW;
#pragma unroll
        for (int i = 0; i < 2; ++i)
          acc[i][k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[ky][i]),
                                                              __builtin_bit_cast(bf16x8_t, bq[idx % (RA + 1)]),
                                                              acc[i][k], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int i = 0; i < 2; ++i) af[ky][i] = an[ky][i];
    };
    using K0 = std::integral_constant<int, 0>;
    using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>;
    block1(0, K0{}, false);
    block1(0, K1{}, false);
    block1(0, K2{}, false);
    block1(1, K0{}, false);
    block1(1, K1{}, false);
    block1(1, K2{}, true);
  }
  // ---- conv1's epilogue into LDS: h = bf16(act1(acc * scale1 + shift1)), zero outside the image
  {
    floatx4 sc[2], sh[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int cl = wc * 32 + i * 16 + c4 * 4;
      sc[i] = *reinterpret_cast<const floatx4*>(d1.scale + cl);
      sh[i] = *reinterpret_cast<const floatx4*>(d1.shift + cl);
    }
    __syncthreads();   // every wave is done reading the input planes
#pragma unroll
    for (int k = 0; k < FPW; ++k) {
      if (k == FPW - 1 && ph) continue;   // (the repeated fragment; wave-uniform)
      const int m = 16 * (FPW * ph + k) + j16;
      const int iy = m / RB_HP, ix = m - RB_HP * iy;
      const int gy = y0 - 1 + iy, gx = x0 - 1 + ix;
      const bool ok = ix < 18 && iy < 18 && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const floatx4 ac = acc[i][k];
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = ac[e] * sc[i][e] + sh[i][e];
          if constexpr (ACT1 == HISEG_ACT_RELU) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        uint2 o;
        o.x = f2bf2(v[0], v[1]);
        o.y = f2bf2(v[2], v[3]);
        if (!ok) o = make_uint2(0u, 0u);
        // channels 16 i + 4 c4 .. + 3 of slice wc: chunk 2 i + c4 / 2, its half c4 % 2
        const int ch = 2 * i + (c4 >> 1);
        *reinterpret_cast<uint2*>(lds_w + RB_PLANE_M * wc + m * 64 + ((ch ^ halo_row_swz(m)) << 4) +
                                  ((c4 & 1) << 3)) = o;
      }
    }
    __syncthreads();   // the intermediate is whole
  }

  // ================================================================================================ conv2
  floatx4 ac2[2][NR2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jr = 0; jr < NR2; ++jr) ac2[i][jr] = floatx4{0.f, 0.f, 0.f, 0.f};
  {
    auto block2 = [&](int sl, auto kxc, bool last) __attribute__((always_inline)) {
      constexpr int KX = decltype(kxc)::value;
      if (!last) load_blk(an, rF2, KX < 2 ? sl : sl + 1, KX < 2 ? KX + 1 : 0);
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int j = ln & 15, cc = ln >> 4;
      // B fragment of ring row 8 ph + r at shift KX: ring pixels (8 ph + r) * 20 + KX + j; the slot swizzle is
      // ((r + (KX + j) / 4) & 1) (5 r and 40 ph have the parities of r and 0)
      const int se = (cc ^ halo_row_swz(KX + j)) << 4;
      const int base = RB_PLANE_M * sl + (NR2 * RB_HP * ph + KX + j) * 64;
      auto rd = [&](int r) __attribute__((always_inline)) -> u32x4 {
        return *reinterpret_cast<const u32x4*>(lds_c + base + ((r & 1) ? (se ^ 32) : se) + r * RB_HP * 64);
      };
      u32x4 bq[3];
      bq[0] = rd(0);
      bq[1] = rd(1);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int r = 0; r < NR2 + 2; ++r) {
        if (r + 2 < NR2 + 2) bq[(r + 2) % 3] = rd(r + 2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int jr = r - ky;
          if (jr >= 0 && jr < NR2) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
              ac2[i][jr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[ky][i]),
                                                                   __builtin_bit_cast(bf16x8_t, bq[r % 3]),
                                                                   ac2[i][jr], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
      if (!last) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int i = 0; i < 2; ++i) af[ky][i] = an[ky][i];
      }
    };
    using K0 = std::integral_constant<int, 0>;
    using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>;
    block2(0, K0{}, false);
    block2(0, K1{}, false);
    block2(0, K2{}, false);
    block2(1, K0{}, false);
    block2(1, K1{}, false);
    block2(1, K2{}, true);
  }
  __syncthreads();   // every wave is done reading the intermediate

  // ---- epilogue through LDS (conv_hwc's, BCO 64): 256 pixel rows x 64 bf16, 16-B chunk c of row r at slot
  // c ^ (r & 7); tile row r = pixel (y0 + r / 16, x0 + r % 16).  The residual tile (x again, warm in L2) arrives by
  // LDS-DMA, each lane turns its accumulator quads into bf16 output quads in place, whole rows leave by 16-B stores.
  constexpr int EROWB = 128, CPR = 8, RPI = 8, SWM = 7, NRI = 256 / (RPI * NW), NST = 256 * CPR / (NW * 64);
  auto px_of = [&](int r) __attribute__((always_inline)) -> int {
    const int y = y0 + (r >> 4), x = x0 + (r & 15);
    return (y < H && x < W) ? (n * H + y) * W + x : -1;
  };
  const __amdgpu_buffer_rsrc_t rR = buf_rsrc(d2.residual, d1.N * H * W * d2.r_cstride * 2);
#pragma unroll
  for (int k = 0; k < NRI; ++k) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int c = ln % CPR;
    const int r = RPI * (w + NW * k) + ln / CPR;
    const int px = px_of(r);
    const unsigned off = px >= 0 ? (unsigned)((px * d2.r_cstride + d2.r_coff + ((c ^ (r & SWM)) * 8)) * 2) : kOobOffset;
    lds_dma16(rR, lds_base + (unsigned)(RPI * (w + NW * k) * EROWB), off);
  }
  floatx4 sc[2], sh[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cl = wc * 32 + i * 16 + c4 * 4;
    sc[i] = *reinterpret_cast<const floatx4*>(d2.scale + cl);
    sh[i] = *reinterpret_cast<const floatx4*>(d2.shift + cl);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  char* tile = lds_w;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jr = 0; jr < NR2; ++jr) {
      const int cl = wc * 32 + i * 16 + c4 * 4;
      const int r = (NR2 * ph + jr) * 16 + j16;
      char* q = tile + r * EROWB + ((((cl >> 3) ^ (r & SWM)) << 4) | ((cl & 4) << 1));
      const floatx4 ac = ac2[i][jr];
      float v[4];
      const uint2 rv = *reinterpret_cast<const uint2*>(q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = ac[e] * sc[i][e] + sh[i][e];
        v[e] += Quad<bf16_t>::get(rv, e);
        if constexpr (ACT2 == HISEG_ACT_RELU) v[e] = v[e] > 0.f ? v[e] : 0.f;
      }
      uint2 o;
      o.x = f2bf2(v[0], v[1]);
      o.y = f2bf2(v[2], v[3]);
      *reinterpret_cast<uint2*>(q) = o;
    }
  __syncthreads();
  uint4 sv[NST];
#pragma unroll
  for (int k = 0; k < NST; ++k) {
    const int idx = t + NW * 64 * k;
    const int r = idx / CPR, c = idx % CPR;
    sv[k] = *reinterpret_cast<const uint4*>(tile + r * EROWB + ((c ^ (r & SWM)) << 4));
  }
  // (num_records: the output's own span, so a lane past the tile -- offset kOobOffset -- is dropped by the hardware)
  const __amdgpu_buffer_rsrc_t rO = buf_rsrc(d2.out, d1.N * H * W * d2.o_cstride * 2);
#pragma unroll
  for (int k = 0; k < NST; ++k) {
    const int idx = t + NW * 64 * k;
    const int r = idx / CPR, c = idx % CPR;
    const int px = px_of(r);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sv[k]), rO,
                                           px >= 0 ? (unsigned)((px * d2.o_cstride + d2.o_coff + 8 * c) * 2) : kOobOffset, 0, 0);
  }
}

// Whether the pair (conv1, conv2) of a ResidualBlock has the fused form: bf16, 3x3 / stride 1 / pad 1, 64 -> 64,
// single source, eval BatchNorm folded, activations none / ReLU, conv2's residual = conv1's input, conv1's output
// nowhere else; every operand under 2 GiB (32-bit buffer offsets).
bool conv_resblock_applies(const hiseg_conv2d_desc& d1, const hiseg_conv2d_desc& d2) {
  for (const hiseg_conv2d_desc* d : {&d1, &d2}) {
    if (d->dtype != HISEG_BF16 || d->out_dtype != HISEG_BF16 || d->weight_frag == nullptr) return false;
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1 || d->convT || d->a_up != 1) return false;
    if (d->Ca != 64 || d->Cb != 0 || d->srcB || d->Cout != 64 || d->Cout_pad != 64 || d->K_pad != 576) return false;
    if (d->act != HISEG_ACT_NONE && d->act != HISEG_ACT_RELU) return false;
    if (d->in_scale || d->mul || d->out2 || d->stats_partial || d->bnb_partial || d->px_scale || d->head2_out ||
        d->head2_w || d->a_gate || d->res_gate || d->workspace)
      return false;
    if (!d->scale || !d->shift || (((uintptr_t)d->scale | (uintptr_t)d->shift | (uintptr_t)d->weight_frag) & 15))
      return false;
    if (d->N != d1.N || d->H != d1.H || d->W != d1.W || d->Ho != d1.H || d->Wo != d1.W) return false;
  }
  if (d1.N <= 0 || d1.H <= 0 || d1.W <= 0) return false;
  if (d1.residual || !d1.srcA || ((uintptr_t)d1.srcA & 15) || ((d1.a_cstride | d1.a_coff) & 7) || d1.a_cstride < 64)
    return false;
  // conv2: its source is the intermediate (never materialised: d2.srcA is not read), its residual is conv1's input
  if (d2.residual != d1.srcA || d2.r_cstride != d1.a_cstride || d2.r_coff != d1.a_coff) return false;
  // a dense 64-channel output at offset 0 (no out= view into a wider tensor)
  if (!d2.out || ((uintptr_t)d2.out & 15) || d2.o_cstride != 64 || d2.o_coff != 0) return false;
  const long long px = (long long)d1.N * d1.H * d1.W;
  if (px * d1.a_cstride * 2 >= 0x7fffffffll || px * d2.o_cstride * 2 >= 0x7fffffffll) return false;
  const long long tiles = (long long)d1.N * ((d1.H + 15) / 16) * ((d1.W + 15) / 16);
  if (tiles >= (1ll << 31)) return false;
  // in place (out == x) is not supported: a tile's halo reads pixels its neighbours write
  if (d2.out == d1.srcA) return false;
  return true;
}

template <int ACT1, int ACT2>
static int launch_resblock(const hiseg_conv2d_desc& d1, const hiseg_conv2d_desc& d2, hipStream_t s) {
  auto kern = conv_resblock_kernel<ACT1, ACT2>;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, RB_LDS);
    attr = true;
  }
  const int tiles = d1.N * ((d1.H + 15) / 16) * ((d1.W + 15) / 16);
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(256), RB_LDS, s, d1, d2);
  return hiseg_check_launch("conv_resblock");
}

// (the caller checked conv_resblock_applies)
int conv_resblock_launch(const hiseg_conv2d_desc& d1, const hiseg_conv2d_desc& d2, hipStream_t s) {
  const bool r1 = d1.act == HISEG_ACT_RELU, r2 = d2.act == HISEG_ACT_RELU;
  return r1 ? (r2 ? launch_resblock<HISEG_ACT_RELU, HISEG_ACT_RELU>(d1, d2, s)
                  : launch_resblock<HISEG_ACT_RELU, HISEG_ACT_NONE>(d1, d2, s))
            : (r2 ? launch_resblock<HISEG_ACT_NONE, HISEG_ACT_RELU>(d1, d2, s)
                  : launch_resblock<HISEG_ACT_NONE, HISEG_ACT_NONE>(d1, d2, s));
}

}  // namespace hiseg
