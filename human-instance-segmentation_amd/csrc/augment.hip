// ROI-safe training augmentation on the GPU (include/hiseg_augment.h): flip, HSV round trip, channel tables,
// k x k filter and the float store of a batch of 8-bit images in one launch, and the ROI target gather of
// flipped samples.
//
// augment_kernel: one workgroup (256 lanes) per 16 x 64 output tile of one sample, 4 consecutive pixels per lane.
//   1. the source bytes of the tile plus its halo (ksize / 2 pixels) are staged into LDS row by row as aligned
//      dwords -- a row segment is contiguous in the source whether or not the sample is flipped;
//   2. with a filter, every tile pixel is flipped / reflected (reflect-101), taken through the HSV round trip and
//      the channel tables ONCE and written to a planar 8-bit tile in LDS; the filter then reads that tile
//      (ksize + 3 bytes per lane, row and channel, as three dword reads);
//   3. without a filter (the common case: blur has p 0.1) the lane colours its own 4 pixels straight from the
//      staged bytes;
//   4. three f32 planes are stored, one 16-byte store per lane and plane where W and the address allow, scalar
//      stores otherwise.
// The sample's six tables, its kernel, the output table and (for HSV) cv2's two division tables sit in LDS.
// Traffic is 3 B read + 12 B written per pixel; no atomics, no host synchronisation.
#include <stddef.h>

#include "common.h"
#include "hiseg_augment.h"
#include "roi_gather.h"

namespace hiseg {

constexpr int kAugTH = 16, kAugTW = 64, kAugR = 3;
constexpr int kAugRows = kAugTH + 2 * kAugR;                   // 22 staged rows at most
constexpr int kAugRawDw = ((kAugTW + 2 * kAugR) * 3 + 3 + 3) / 4;   // 54 dwords: 210 bytes + alignment shift
constexpr int kAugPixDw = (kAugTW + 2 * kAugR + 3) / 4;        // 18 dwords = 72 bytes per planar tile row
static_assert(kAugPixDw * 4 >= kAugTW - 4 + 12, "a lane reads 12 bytes from its first pixel");
static_assert(offsetof(hiseg_aug_sample, hsv_lut) == 16 && offsetof(hiseg_aug_sample, rgb_lut) == 16 + 768 &&
                  offsetof(hiseg_aug_sample, kernel) == 16 + 1536 && sizeof(hiseg_aug_sample) == 16 + 1536 + 196,
              "hiseg_aug_sample layout");

// cv2 color_hsv.simd.hpp RGB2HSV_b: sdiv_table[i] = saturate_cast<int>((255 << 12) / (1. * i)),
// hdiv_table180[i] = saturate_cast<int>((180 << 12) / (6. * i)); saturate_cast rounds half to even.  Both
// quotients are rationals whose distance from a tie is 0 or at least 1 / 510, so exact integer rounding gives
// the double result.
struct AugDivTab { int v[256]; };
constexpr AugDivTab aug_div_tab(int n) {
  AugDivTab t{};
  for (int i = 1; i < 256; ++i) {
    int q = n / i;
    const int rem = n % i;
    if (2 * rem > i || (2 * rem == i && (q & 1))) ++q;
    t.v[i] = q;
  }
  return t;
}
__device__ const AugDivTab kAugSdiv = aug_div_tab(255 << 12);
__device__ const AugDivTab kAugHdiv = aug_div_tab((180 << 12) / 6);

__device__ __forceinline__ float aug_sel4(float t0, float t1, float t2, float t3, int i) {
  return i == 0 ? t0 : (i == 1 ? t1 : (i == 2 ? t2 : t3));
}

// (hipcc's __fmul_rn / __fadd_rn / __fsub_rn are plain operators compiled with the HIP default -ffp-contract=fast, and
// fuse into FMAs once inlined; plain operators under the pragma are what keeps each operation rounded on its own.)
__device__ __forceinline__ int aug_u8(float x) {   // saturate_cast<uchar>(x * 255.f)
#pragma clang fp contract(off)
  const float q = rintf(x * 255.f);
  return q < 0.f ? 0 : (q > 255.f ? 255 : (int)q);
}

// cv2's 8-bit RGB -> HSV (H in 0..179), the three tables, cv2's 8-bit HSV -> RGB in f32 (no FMA contraction:
// every product and sum is rounded on its own, as the library's scalar code).
__device__ __forceinline__ void aug_hsv(int& r, int& g, int& b, const uint8_t* lut, const int* sdiv, const int* hdiv) {
#pragma clang fp contract(off)
  const int v0 = max(r, max(g, b)), d = v0 - min(r, min(g, b));
  int s = (d * sdiv[v0] + 2048) >> 12;
  int h = v0 == r ? g - b : (v0 == g ? b - r + 2 * d : r - g + 4 * d);
  h = (h * hdiv[d] + 2048) >> 12;
  if (h < 0) h += 180;
  h = lut[h];
  s = lut[256 + s];
  const int v = lut[512 + v0];
  const float inv255 = 1.f / 255.f;
  const float S = (float)s * inv255, V = (float)v * inv255;
  float fb = V, fg = V, fr = V;
  if (s != 0) {
    const float hscale = 6.f / 180.f;
    float hh = (float)h * hscale;
    while (hh >= 6.f) hh -= 6.f;
    const float kf = floorf(hh);
    const int k = (int)kf;
    const float f = hh - kf;
    const float oms = 1.f - S, sf = S * f;
    const float t0 = V, t1 = V * oms, t2 = V * (1.f - sf), t3 = V * (oms + sf);
    // sector_data {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}: (b, g, r) = t[idx[k]], 2 bits per sector
    constexpr unsigned kB = 1u | 1u << 2 | 3u << 4 | 0u << 6 | 0u << 8 | 2u << 10;
    constexpr unsigned kG = 3u | 0u << 2 | 0u << 4 | 2u << 6 | 1u << 8 | 1u << 10;
    constexpr unsigned kR = 0u | 2u << 2 | 1u << 4 | 1u << 6 | 3u << 8 | 0u << 10;
    fb = aug_sel4(t0, t1, t2, t3, (kB >> (2 * k)) & 3);
    fg = aug_sel4(t0, t1, t2, t3, (kG >> (2 * k)) & 3);
    fr = aug_sel4(t0, t1, t2, t3, (kR >> (2 * k)) & 3);
  }
  r = aug_u8(fr);
  g = aug_u8(fg);
  b = aug_u8(fb);
}

struct AugShared {
  uint32_t raw[kAugRows][kAugRawDw];      // staged source bytes, row segment starting at the aligned address
  uint32_t pix[3][kAugRows][kAugPixDw];   // planar recoloured tile (filter input)
  uint32_t lut[384];                      // hsv_lut[3][256] then rgb_lut[3][256]
  float kern[49];
  float otab[256];
  int sdiv[256], hdiv[256];
  int shift[kAugRows];
};

// Stages 1-3 for the pixel at staged row `row`, flipped-image column px (inside [pl, ph]): reads its 3 bytes from
// the staged segment, which starts at source column sl.
__device__ __forceinline__ void aug_colour(const AugShared& sh, int row, int px, int W, int sl, bool flip, bool hsv,
                                           int& r, int& g, int& b) {
  const int sx = flip ? W - 1 - px : px;
  const uint8_t* p = reinterpret_cast<const uint8_t*>(sh.raw[row]) + (sx - sl) * 3 + sh.shift[row];
  r = p[0];
  g = p[1];
  b = p[2];
  const uint8_t* lut = reinterpret_cast<const uint8_t*>(sh.lut);
  if (hsv) aug_hsv(r, g, b, lut, sh.sdiv, sh.hdiv);
  r = lut[768 + r];
  g = lut[1024 + g];
  b = lut[1280 + b];
}

__device__ __forceinline__ void aug_store(float* out, long long o, int x0, int W, const float* v) {
  float* p = out + o;
  if (x0 + 3 < W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < W) p[k] = v[k];
  }
}

// KS x KS correlation of the planar tile for this lane's 4 pixels (tile row ty .. ty + KS - 1, tile columns
// x4 .. x4 + KS + 2), f32 sum in row-major tap order, then the output table.
template <int KS>
__device__ __forceinline__ void aug_filter(const AugShared& sh, int ty, int x4, float (*res)[4]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const uint32_t* rowp = &sh.pix[c][ty + i][x4 >> 2];
      const uint32_t w[3] = {rowp[0], rowp[1], rowp[2]};
      float v[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) v[j] = (float)((w[j >> 2] >> (8 * (j & 3))) & 255u);
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        const float kw = sh.kern[i * KS + j];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(kw, v[j + k], acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float q = rintf(acc[k]);
      res[c][k] = sh.otab[q < 0.f ? 0 : (q > 255.f ? 255 : (int)q)];
    }
  }
}

__global__ void __launch_bounds__(256) augment_kernel(const uint8_t* __restrict__ src,
                                                      const hiseg_aug_sample* __restrict__ samples,
                                                      const float* __restrict__ out_table, int H, int W,
                                                      long long total_bytes, float* __restrict__ out) {
  __shared__ AugShared sh;
  const int t = threadIdx.x, b = blockIdx.z;
  const int tx0 = blockIdx.x * kAugTW, ty0 = blockIdx.y * kAugTH;
  const hiseg_aug_sample* s = samples + b;
  const bool flip = s->flip != 0, hsv = s->hsv != 0;
  int ks = s->ksize;
  if (ks != 3 && ks != 5 && ks != 7) ks = 0;
  const int r = ks >> 1;

  const uint32_t* lut32 = reinterpret_cast<const uint32_t*>(&s->hsv_lut[0][0]);
  for (int i = t; i < 384; i += 256) sh.lut[i] = lut32[i];
  sh.otab[t] = out_table[t];
  if (ks && t < ks * ks) sh.kern[t] = s->kernel[t];
  if (hsv) {
    sh.sdiv[t] = kAugSdiv.v[t];
    sh.hdiv[t] = kAugHdiv.v[t];
  }

  // the tile's columns of the flipped image [pl, ph] (halo included, clipped to the image: a reflected column
  // lies inside it) are the source columns [sl, sl + ncol)
  const int pl = max(0, tx0 - r), ph = min(W - 1, tx0 + kAugTW - 1 + r);
  const int sl = flip ? W - 1 - ph : pl, ncol = ph - pl + 1;
  const int nrow = min(kAugTH, H - ty0) + 2 * r;
  const int ndmax = (ncol * 3 + 3 + 3) >> 2;   // <= kAugRawDw
  const uintptr_t lo = reinterpret_cast<uintptr_t>(src), hi = lo + (uintptr_t)total_bytes;
  for (int idx = t; idx < nrow * ndmax; idx += 256) {
    const int row = idx / ndmax, i = idx - row * ndmax;
    int y = ty0 + row - r;                      // reflect-101; H >= 4 > r keeps it inside
    y = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y);
    const uintptr_t g = lo + (uintptr_t)((((long long)b * H + y) * W + sl) * 3);
    const int shift = (int)(g & 3);
    if (i == 0) sh.shift[row] = shift;
    if (i * 4 < ncol * 3 + shift) {
      const uintptr_t a = g - shift + (uintptr_t)i * 4;
      uint32_t v = 0;
      if (a >= lo && a + 4 <= hi) {
        v = *reinterpret_cast<const uint32_t*>(a);
      } else {   // the dword straddles an end of the buffer: only the bytes inside it
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (a + k >= lo && a + k < hi) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(a + k)) << (8 * k);
      }
      sh.raw[row][i] = v;
    }
  }
  __syncthreads();

  const int ty = t >> 4, x4 = (t & 15) << 2;
  const int y = ty0 + ty, x0 = tx0 + x4;
  float res[3][4];
  if (ks == 0) {
    if (y >= H || x0 >= W) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int cr, cg, cb;
      aug_colour(sh, ty, min(x0 + k, W - 1), W, sl, flip, hsv, cr, cg, cb);
      res[0][k] = sh.otab[cr];
      res[1][k] = sh.otab[cg];
      res[2][k] = sh.otab[cb];
    }
  } else {
    const int tw2 = kAugTW + 2 * r;
    uint8_t* pix = reinterpret_cast<uint8_t*>(sh.pix);
    for (int idx = t; idx < nrow * tw2; idx += 256) {
      const int row = idx / tw2, lx = idx - row * tw2;
      int px = tx0 + lx - r;
      px = px < 0 ? -px : (px >= W ? 2 * W - 2 - px : px);
      px = min(max(px, pl), ph);   // columns past the tile's last image column feed no stored output
      int cr, cg, cb;
      aug_colour(sh, row, px, W, sl, flip, hsv, cr, cg, cb);
      const int o = row * (kAugPixDw * 4) + lx;
      pix[o] = (uint8_t)cr;
      pix[o + kAugRows * kAugPixDw * 4] = (uint8_t)cg;
      pix[o + 2 * kAugRows * kAugPixDw * 4] = (uint8_t)cb;
    }
    __syncthreads();
    if (y >= H || x0 >= W) return;
    if (ks == 3) aug_filter<3>(sh, ty, x4, res);
    else if (ks == 5) aug_filter<5>(sh, ty, x4, res);
    else aug_filter<7>(sh, ty, x4, res);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) aug_store(out, (((long long)b * 3 + c) * H + y) * W + x0, x0, W, res[c]);
}

__global__ void __launch_bounds__(256) roi_targets_flip_kernel(const uint8_t* masks, const hiseg_roi_target_desc* descs,
                                                               const int* flip, int mh, int mw, long long* out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (idx >= mh * mw) return;
  const hiseg_roi_target_desc d = descs[b];
  out[(long long)b * mh * mw + idx] = roi_target_class(masks, d, mh, mw, idx, flip[b] != 0);
}

}  // namespace hiseg

using namespace hiseg;

extern "C" int hiseg_aug_struct_size(void) { return (int)sizeof(hiseg_aug_sample); }

extern "C" int hiseg_aug_validate(const hiseg_aug_sample* host_samples, int B) {
  HISEG_REQUIRE(host_samples && B > 0, HISEG_ERR_BAD_ARG, "aug_validate: null or empty");
  for (int b = 0; b < B; ++b) {
    const hiseg_aug_sample& s = host_samples[b];
    HISEG_REQUIRE(s.ksize == 0 || s.ksize == 3 || s.ksize == 5 || s.ksize == 7, HISEG_ERR_BAD_ARG,
                  "aug_validate: sample %d: ksize %d (0, 3, 5 or 7)", b, s.ksize);
    HISEG_REQUIRE((s.flip == 0 || s.flip == 1) && (s.hsv == 0 || s.hsv == 1), HISEG_ERR_BAD_ARG,
                  "aug_validate: sample %d: flip %d / hsv %d (0 or 1)", b, s.flip, s.hsv);
  }
  return HISEG_OK;
}

extern "C" int hiseg_augment_fwd(const unsigned char* src, const hiseg_aug_sample* samples, const float* out_table,
                                 int B, int H, int W, float* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(src && samples && out_table && out, HISEG_ERR_BAD_ARG, "augment_fwd: null");
  HISEG_REQUIRE(B > 0 && B <= 65535 && H >= 4 && W >= 4 && (H + kAugTH - 1) / kAugTH <= 65535, HISEG_ERR_BAD_SHAPE,
                "augment_fwd: shape B %d H %d W %d (H, W >= 4)", B, H, W);
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(samples) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                HISEG_ERR_BAD_ARG, "augment_fwd: samples / out not 4-byte aligned");
  const dim3 g((unsigned)((W + kAugTW - 1) / kAugTW), (unsigned)((H + kAugTH - 1) / kAugTH), (unsigned)B);
  hipLaunchKernelGGL(augment_kernel, g, dim3(256), 0, (hipStream_t)stream, src, samples, out_table, H, W,
                     (long long)B * H * W * 3, out);
  return hiseg_check_launch("augment_fwd");
}

extern "C" int hiseg_roi_targets_flip(const unsigned char* masks, const hiseg_roi_target_desc* descs, const int* flip,
                                      int B, int mh, int mw, long long* out, hiseg_stream_t stream) {
  HISEG_REQUIRE(masks && descs && flip && out, HISEG_ERR_BAD_ARG, "roi_targets_flip: null");
  HISEG_REQUIRE(B > 0 && B <= 65535 && mh > 0 && mw > 0 && (long long)mh * mw < (1ll << 31), HISEG_ERR_BAD_SHAPE,
                "roi_targets_flip: shape");
  hipLaunchKernelGGL(roi_targets_flip_kernel, dim3((unsigned)(((long long)mh * mw + 255) / 256), (unsigned)B), dim3(256),
                     0, (hipStream_t)stream, masks, descs, flip, mh, mw, out);
  return hiseg_check_launch("roi_targets_flip");
}
