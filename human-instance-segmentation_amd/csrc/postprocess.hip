// Mask post-processing (include/hiseg_post.h): edge smoothing and the bilateral-filter family on f32 planes.
//
// One kernel shape serves every stencil chain.  A workgroup owns a tile of one plane and keeps the tile plus a
// halo of R pixels (the "region") in LDS, in two buffers; every stage / iteration reads one buffer and writes
// the other with a barrier in between, so a plane is read from HBM once and written once (8 bytes / pixel).
//   resident form: the tile is the whole plane, R = 0, one workgroup per plane.  Taken when the two buffers fit
//                  the 160 KB of LDS (H*W <= kResidentPx = 20480: the 64x48 and 128x96 instance masks).
//   tiled form:    64x64 tiles, R = iterations * radius (summed radii for the morphological chain) <= kMaxHalo;
//                  every tile recomputes its halo, which shrinks by one radius per stage.
// Padding: a region pixel that lies outside the IMAGE is rewritten by every stage with the pad value of the
// stage that reads it next (0 for a zero-padded convolution, +inf / -inf for a min / max that must not see the
// padding), so the image border behaves as the reference's padding at every iteration, not only the first.  A
// tap outside the REGION reads that same pad value: it only feeds pixels of the halo that the central tile never
// depends on.  Both forms therefore compute the tile's pixels from the same values in the same order: they agree
// bit for bit, and N iterations in one launch equal N launches of one.
//
// No MFMA: the kernels are LDS-read / VALU work over a bandwidth-sized stream.
#include <math.h>
#include <hip/hip_fp16.h>
#include "common.h"
#include "hiseg_post.h"

namespace hiseg {

constexpr int kPostLds = 160 * 1024;              // bytes of LDS a workgroup may use on gfx950
constexpr int kResidentPx = kPostLds / 8;         // two f32 buffers per pixel
constexpr int kPostTile = 64;                     // tiled form: tile edge
constexpr int kMaxHalo = 32;                      // (64 + 2*32)^2 * 8 B = 128 KB
constexpr int kMaxK = 9;

struct PostGeom {
  int H, W;          // plane
  int TH, TW;        // tile
  int tiles_x, tiles;  // tiles per row / per plane
  int R;             // halo
};

struct PostWeights { float w[kMaxK * kMaxK]; };

// The region of this workgroup: origin in image coordinates and size.
struct Region {
  int y0, x0, RH, RW, H, W;
  __device__ __forceinline__ int size() const { return RH * RW; }
  __device__ __forceinline__ bool in_image(int ly, int lx) const {
    return (unsigned)(y0 + ly) < (unsigned)H && (unsigned)(x0 + lx) < (unsigned)W;
  }
  __device__ __forceinline__ float tap(const float* buf, int ly, int lx, float pad) const {
    return ((unsigned)ly < (unsigned)RH && (unsigned)lx < (unsigned)RW) ? buf[ly * RW + lx] : pad;
  }
};

__device__ __forceinline__ Region region_of(const PostGeom& g, int tile) {
  Region r;
  r.y0 = (tile / g.tiles_x) * g.TH - g.R;
  r.x0 = (tile % g.tiles_x) * g.TW - g.R;
  r.RH = g.TH + 2 * g.R;
  r.RW = g.TW + 2 * g.R;
  r.H = g.H;
  r.W = g.W;
  return r;
}

// Store the central tile (clipped to the image) of `buf`; THRESH: 1.0 where value > thr, else 0.0.
template <bool THRESH>
__device__ __forceinline__ void store_tile(const float* buf, const Region& r, const PostGeom& g, float* out, float thr) {
  for (int i = threadIdx.x; i < g.TH * g.TW; i += blockDim.x) {
    const int ty = i / g.TW, tx = i - ty * g.TW;
    const int gy = r.y0 + g.R + ty, gx = r.x0 + g.R + tx;
    if (gy < g.H && gx < g.W) {
      const float v = buf[(ty + g.R) * r.RW + tx + g.R];
      out[(long long)gy * g.W + gx] = THRESH ? (v > thr ? 1.f : 0.f) : v;
    }
  }
}

// m*(1-e) + b*e with every operation rounded to f32 on its own, in this order (edge_smoothing.py:74).  The
// reference's decision at a pixel whose blend is exactly 0.5 (the centre of a one-pixel line: e = sigmoid(18)
// rounds to 1.0f) depends on it, so no contraction into an FMA and no algebraic rewrite.
__device__ __forceinline__ float blend_f32(float m, float b, float e) {
#pragma clang fp contract(off)
  const float keep = m * (1.0f - e);
  const float blur = b * e;
  return keep + blur;
}

// 1 / (1 + exp(-x)) as torch evaluates it in f32: the accurate expf and the correctly rounded division.
__device__ __forceinline__ float sigmoid_f32(float x) {
#pragma clang fp contract(off)
  return 1.0f / (1.0f + expf(-x));
}

// BinaryMaskEdgeSmoothing.forward x iterations.  MODE kEdgeClasses: the input is [B,3,H,W] scores and plane
// p = b*3 + c is the mask argmax == c (first maximum wins); kEdgeBinarize: the mask is x > 0.5
// (edge_smoothing.py:144).  Either is formed while the region is loaded.
constexpr int kEdgePlain = 0, kEdgeClasses = 1, kEdgeBinarize = 2;
template <int MODE>
__global__ void __launch_bounds__(1024) edge_smooth_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                           PostGeom g, float threshold, float blur_strength,
                                                           int iterations) {
  extern __shared__ float post_lds[];
  const long long plane = blockIdx.x / g.tiles;
  const Region r = region_of(g, (int)(blockIdx.x % g.tiles));
  const long long HW = (long long)g.H * g.W;
  const int n = r.size();
  float* a = post_lds;
  float* b = post_lds + n;

  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ly = i / r.RW, lx = i - ly * r.RW;
    float v = 0.f;
    if (r.in_image(ly, lx)) {
      const long long px = (long long)(r.y0 + ly) * g.W + (r.x0 + lx);
      if constexpr (MODE == kEdgeClasses) {
        const float* s = x + (plane / 3) * 3 * HW + px;
        const float s0 = s[0], s1 = s[HW], s2 = s[2 * HW];
        int best = 0;
        float bv = s0;
        if (s1 > bv) { bv = s1; best = 1; }
        if (s2 > bv) { best = 2; }
        v = best == (int)(plane % 3) ? 1.f : 0.f;
      } else {
        v = x[plane * HW + px];
        if constexpr (MODE == kEdgeBinarize) v = v > 0.5f ? 1.f : 0.f;
      }
    }
    a[i] = v;
  }
  __syncthreads();

  for (int it = 0; it < iterations; ++it) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int ly = i / r.RW, lx = i - ly * r.RW;
      float o = 0.f;
      if (r.in_image(ly, lx)) {
        const float c = a[i];
        const float edge = (r.tap(a, ly - 1, lx, 0.f) + r.tap(a, ly + 1, lx, 0.f)) +
                           (r.tap(a, ly, lx - 1, 0.f) + r.tap(a, ly, lx + 1, 0.f));
        const float corner = (r.tap(a, ly - 1, lx - 1, 0.f) + r.tap(a, ly - 1, lx + 1, 0.f)) +
                             (r.tap(a, ly + 1, lx - 1, 0.f) + r.tap(a, ly + 1, lx + 1, 0.f));
        const float lap = 8.f * c - (edge + corner);
        const float blurred = 0.25f * c + (0.125f * edge + 0.0625f * corner);
        const float e = sigmoid_f32(fabsf(lap) * blur_strength);
        o = blend_f32(c, blurred, e) > threshold ? 1.f : 0.f;
      }
      b[i] = o;
    }
    __syncthreads();
    float* t = a; a = b; b = t;
  }
  store_tile<false>(a, r, g, out + plane * HW, 0.f);
}

// x <- w*f + (1-w)*x with f = G*x, w = exp(-max(G*x^2 - f^2, 0) * gain); G = K x K weights, zero padding.
template <int K>
__global__ void __launch_bounds__(1024) var_gated_blur_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                              PostGeom g, PostWeights wt, float gain, int clamp_input,
                                                              int threshold_output, float threshold, int iterations) {
  extern __shared__ float post_lds[];
  constexpr int P = K / 2;
  const long long plane = blockIdx.x / g.tiles;
  const Region r = region_of(g, (int)(blockIdx.x % g.tiles));
  const long long HW = (long long)g.H * g.W;
  const int n = r.size();
  float* a = post_lds;
  float* b = post_lds + n;

  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ly = i / r.RW, lx = i - ly * r.RW;
    float v = 0.f;
    if (r.in_image(ly, lx)) {
      v = x[plane * HW + (long long)(r.y0 + ly) * g.W + (r.x0 + lx)];
      if (clamp_input) v = fminf(fmaxf(v, 0.f), 1.f);
    }
    a[i] = v;
  }
  __syncthreads();

  for (int it = 0; it < iterations; ++it) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int ly = i / r.RW, lx = i - ly * r.RW;
      float o = 0.f;
      if (r.in_image(ly, lx)) {
        float f = 0.f, q = 0.f;
#pragma unroll
        for (int dy = 0; dy < K; ++dy) {
#pragma unroll
          for (int dx = 0; dx < K; ++dx) {
            const float v = r.tap(a, ly + dy - P, lx + dx - P, 0.f);
            const float wv = wt.w[dy * K + dx] * v;
            f += wv;
            q = fmaf(wv, v, q);
          }
        }
        const float var = fmaxf(q - f * f, 0.f);
        const float w = expf(-var * gain);
        o = w * f + (1.f - w) * a[i];
      }
      b[i] = o;
    }
    __syncthreads();
    float* t = a; a = b; b = t;
  }
  if (threshold_output) store_tile<true>(a, r, g, out + plane * HW, threshold);
  else store_tile<false>(a, r, g, out + plane * HW, 0.f);
}

// One min (MAX = false) or max stage over an m x m window that never sees the padding: pixels outside the image
// hold the identity of the stage (+inf / -inf), written by the stage before as `next_pad`.
template <bool MAX>
__device__ __forceinline__ void minmax_stage(const float* a, float* b, const Region& r, int rad, float next_pad) {
  const float ident = MAX ? -INFINITY : INFINITY;
  const int n = r.size();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ly = i / r.RW, lx = i - ly * r.RW;
    float o = next_pad;
    if (r.in_image(ly, lx)) {
      float m = ident;
      for (int dy = -rad; dy <= rad; ++dy)
        for (int dx = -rad; dx <= rad; ++dx) {
          const float v = r.tap(a, ly + dy, lx + dx, ident);
          m = MAX ? fmaxf(m, v) : fminf(m, v);
        }
      o = m;
    }
    b[i] = o;
  }
  __syncthreads();
}

// MorphologicalBilateralFilter.forward: clamp, open (min, max), K x K Gaussian with zero padding, close (max,
// min), > 0.5.
template <int K>
__global__ void __launch_bounds__(1024) morph_bilateral_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                               PostGeom g, PostWeights wt, int morph_rad) {
  extern __shared__ float post_lds[];
  constexpr int P = K / 2;
  const long long plane = blockIdx.x / g.tiles;
  const Region r = region_of(g, (int)(blockIdx.x % g.tiles));
  const long long HW = (long long)g.H * g.W;
  const int n = r.size();
  float* a = post_lds;
  float* b = post_lds + n;

  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ly = i / r.RW, lx = i - ly * r.RW;
    float v = INFINITY;
    if (r.in_image(ly, lx))
      v = fminf(fmaxf(x[plane * HW + (long long)(r.y0 + ly) * g.W + (r.x0 + lx)], 0.f), 1.f);
    a[i] = v;
  }
  __syncthreads();
  minmax_stage<false>(a, b, r, morph_rad, -INFINITY);   // erode
  minmax_stage<true>(b, a, r, morph_rad, 0.f);          // dilate -> opened, zero padded for the convolution
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ly = i / r.RW, lx = i - ly * r.RW;
    float o = -INFINITY;
    if (r.in_image(ly, lx)) {
      float f = 0.f;
#pragma unroll
      for (int dy = 0; dy < K; ++dy) {
#pragma unroll
        for (int dx = 0; dx < K; ++dx) f = fmaf(wt.w[dy * K + dx], r.tap(a, ly + dy - P, lx + dx - P, 0.f), f);
      }
      o = f;
    }
    b[i] = o;
  }
  __syncthreads();
  minmax_stage<true>(b, a, r, morph_rad, INFINITY);     // dilate
  minmax_stage<false>(a, b, r, morph_rad, 0.f);         // erode -> closed
  store_tile<true>(b, r, g, out + plane * HW, 0.5f);
}

// BilateralFilter.forward: reflect padding, weight = spatial * exp(-(p - c)^2 * inv2sr), sum(p*w) / (sum(w) + 1e-8).
// One thread per output pixel straight from memory (the taps of neighbouring lanes share cache lines).
template <int K>
__global__ void __launch_bounds__(256) bilateral_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                        long long total, int H, int W, PostWeights wt, float inv2sr) {
  constexpr int P = K / 2;
  const long long HW = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long plane = i / HW;
    const int px = (int)(i - plane * HW);
    const int y = px / W, xx = px - y * W;
    const float* src = x + plane * HW;
    const float c = src[px];
    float sw = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
      int yy = y + dy - P;
      yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
#pragma unroll
      for (int dx = 0; dx < K; ++dx) {
        int xq = xx + dx - P;
        xq = xq < 0 ? -xq : (xq >= W ? 2 * (W - 1) - xq : xq);
        const float p = src[yy * W + xq];
        const float d = p - c;
        const float w = wt.w[dy * K + dx] * expf(-(d * d) * inv2sr);
        sw += w;
        sv = fmaf(p, w, sv);
      }
    }
    out[i] = sv / (sw + 1e-8f);
  }
}

}  // namespace hiseg

using namespace hiseg;

namespace {

struct PostPlan {
  PostGeom g;
  unsigned grid, block;
  size_t lds;
};

bool post_resident(int H, int W, int force_tiled) { return !force_tiled && (long long)H * W <= kResidentPx; }

// Shape checks and the launch plan shared by the LDS kernels; `halo` is the tiled form's R.
int post_plan(const char* what, const void* x, const void* out, long long NC, int H, int W, int halo, int force_tiled,
              PostPlan* p) {
  HISEG_REQUIRE(NC >= 0 && H >= 0 && W >= 0 && (long long)H * W <= 0x7fffffffll, HISEG_ERR_BAD_SHAPE,
                "%s: planes %lld H %d W %d", what, NC, H, W);
  PostGeom& g = p->g;
  g.H = H;
  g.W = W;
  p->grid = 0;
  if (NC == 0 || H == 0 || W == 0) return HISEG_OK;   // nothing to do (an empty tensor has no address)
  HISEG_REQUIRE(x && out, HISEG_ERR_BAD_ARG, "%s: null pointer", what);
  if (post_resident(H, W, force_tiled)) {
    g.TH = H; g.TW = W; g.tiles_x = 1; g.tiles = 1; g.R = 0;
    const int px = H * W;
    p->block = px >= 1024 ? 1024u : (unsigned)((px + 63) / 64 * 64);
  } else {
    HISEG_REQUIRE(halo <= kMaxHalo, HISEG_ERR_BAD_ARG,
                  "%s: the tiled form holds a halo of at most %d pixels, iterations x radius is %d "
                  "(hiseg_post_max_iterations; split the launch)", what, kMaxHalo, halo);
    g.TH = g.TW = kPostTile;
    g.R = halo;
    g.tiles_x = (W + kPostTile - 1) / kPostTile;
    g.tiles = g.tiles_x * ((H + kPostTile - 1) / kPostTile);
    p->block = 256;
  }
  const long long blocks = NC * g.tiles;
  HISEG_REQUIRE(blocks <= 0x7fffffffll, HISEG_ERR_BAD_SHAPE, "%s: %lld workgroups", what, blocks);
  p->grid = (unsigned)blocks;
  p->lds = (size_t)(g.TH + 2 * g.R) * (g.TW + 2 * g.R) * 2 * sizeof(float);
  return HISEG_OK;
}

// Normalised Gaussian as the outer product of the normalised 1-D kernel (bilateral_filter.py:149-152, 334-345,
// 438-445), or the unnormalised 2-D spatial kernel of BilateralFilter (45-56).
void gaussian_weights(int k, float sigma, bool normalised, PostWeights* w) {
  float g1[kMaxK], sum = 0.f;
  for (int i = 0; i < k; ++i) {
    const float c = (float)i - (float)(k - 1) / 2.f;
    g1[i] = expf(-(c * c) / (2.f * sigma * sigma));
    sum += g1[i];
  }
  for (int y = 0; y < k; ++y)
    for (int x = 0; x < k; ++x) {
      if (normalised) {
        w->w[y * k + x] = (g1[y] / sum) * (g1[x] / sum);
      } else {
        const float cy = (float)y - (float)(k - 1) / 2.f, cx = (float)x - (float)(k - 1) / 2.f;
        w->w[y * k + x] = expf(-(cx * cx + cy * cy) / (2.f * sigma * sigma));
      }
    }
  for (int i = k * k; i < kMaxK * kMaxK; ++i) w->w[i] = 0.f;
}

bool good_k(int k) { return k >= 3 && k <= kMaxK && (k & 1); }

template <typename Kern, typename... Args>
void post_launch(Kern kern, const PostPlan& p, hipStream_t s, Args... args) {
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kPostLds);
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.block), p.lds, s, args...);
}

int edge_smooth(const char* what, int mode, const float* x, float* out, long long NC, int H, int W,
                float threshold, float blur_strength, int iterations, int force_tiled, hiseg_stream_t stream) {
  HISEG_REQUIRE(iterations >= 1, HISEG_ERR_BAD_ARG, "%s: iterations %d", what, iterations);
  PostPlan p;
  const int st = post_plan(what, x, out, NC, H, W, iterations > kMaxHalo ? kMaxHalo + 1 : iterations, force_tiled, &p);
  if (st != HISEG_OK || p.grid == 0) return st;
  hipStream_t s = (hipStream_t)stream;
  if (mode == kEdgeClasses)
    post_launch(edge_smooth_kernel<kEdgeClasses>, p, s, x, out, p.g, threshold, blur_strength, iterations);
  else if (mode == kEdgeBinarize)
    post_launch(edge_smooth_kernel<kEdgeBinarize>, p, s, x, out, p.g, threshold, blur_strength, iterations);
  else
    post_launch(edge_smooth_kernel<kEdgePlain>, p, s, x, out, p.g, threshold, blur_strength, iterations);
  return hiseg_check_launch(what);
}

}  // namespace

extern "C" int hiseg_post_max_iterations(int H, int W, int radius, int force_tiled) {
  if (radius < 1 || post_resident(H, W, force_tiled)) return 0x7fffffff;
  return kMaxHalo / radius;
}

extern "C" int hiseg_edge_smooth_fwd(const float* x, float* out, long long NC, int H, int W, float threshold,
                                     float blur_strength, int iterations, int binarize_input, int force_tiled,
                                     hiseg_stream_t stream) {
  return edge_smooth("edge_smooth", binarize_input ? kEdgeBinarize : kEdgePlain, x, out, NC, H, W, threshold,
                     blur_strength, iterations, force_tiled, stream);
}

extern "C" int hiseg_class_edge_smooth_fwd(const float* scores, float* out, long long B, int H, int W,
                                           float threshold, float blur_strength, int iterations, int force_tiled,
                                           hiseg_stream_t stream) {
  HISEG_REQUIRE(B >= 0 && B <= 0x7fffffffll, HISEG_ERR_BAD_SHAPE, "class_edge_smooth: batch %lld", B);
  return edge_smooth("class_edge_smooth", kEdgeClasses, scores, out, B * 3, H, W, threshold, blur_strength, iterations,
                     force_tiled, stream);
}

extern "C" int hiseg_var_gated_blur_fwd(const float* x, float* out, long long NC, int H, int W, int kernel_size,
                                        float sigma_spatial, float gain, int clamp_input, int threshold_output,
                                        float threshold, int iterations, int force_tiled, hiseg_stream_t stream) {
  HISEG_REQUIRE(good_k(kernel_size), HISEG_ERR_BAD_ARG, "var_gated_blur: kernel_size %d (odd, 3..9)", kernel_size);
  HISEG_REQUIRE(iterations >= 1 && sigma_spatial > 0.f, HISEG_ERR_BAD_ARG, "var_gated_blur: iterations %d sigma %g",
                iterations, (double)sigma_spatial);
  PostPlan p;
  const long long halo = (long long)iterations * (kernel_size / 2);
  const int st = post_plan("var_gated_blur", x, out, NC, H, W, halo > kMaxHalo ? kMaxHalo + 1 : (int)halo,
                           force_tiled, &p);
  if (st != HISEG_OK || p.grid == 0) return st;
  PostWeights wt;
  gaussian_weights(kernel_size, sigma_spatial, true, &wt);
  hipStream_t s = (hipStream_t)stream;
#define HISEG_VGB(K)                                                                                          \
  case K:                                                                                                     \
    post_launch(var_gated_blur_kernel<K>, p, s, x, out, p.g, wt, gain, clamp_input, threshold_output, threshold, \
                iterations);                                                                                  \
    break;
  switch (kernel_size) { HISEG_VGB(3) HISEG_VGB(5) HISEG_VGB(7) HISEG_VGB(9) }
#undef HISEG_VGB
  return hiseg_check_launch("var_gated_blur");
}

extern "C" int hiseg_morph_bilateral_fwd(const float* x, float* out, long long NC, int H, int W, int kernel_size,
                                         float sigma, int morph_size, int force_tiled, hiseg_stream_t stream) {
  HISEG_REQUIRE(good_k(kernel_size), HISEG_ERR_BAD_ARG, "morph_bilateral: kernel_size %d (odd, 3..9)", kernel_size);
  HISEG_REQUIRE(morph_size >= 1 && morph_size <= kMaxK && (morph_size & 1) && sigma > 0.f, HISEG_ERR_BAD_ARG,
                "morph_bilateral: morph_size %d (odd, 1..9) sigma %g", morph_size, (double)sigma);
  PostPlan p;
  const int st = post_plan("morph_bilateral", x, out, NC, H, W, 4 * (morph_size / 2) + kernel_size / 2, force_tiled,
                           &p);
  if (st != HISEG_OK || p.grid == 0) return st;
  PostWeights wt;
  gaussian_weights(kernel_size, sigma, true, &wt);
  hipStream_t s = (hipStream_t)stream;
#define HISEG_MB(K)                                                                  \
  case K:                                                                            \
    post_launch(morph_bilateral_kernel<K>, p, s, x, out, p.g, wt, morph_size / 2);   \
    break;
  switch (kernel_size) { HISEG_MB(3) HISEG_MB(5) HISEG_MB(7) HISEG_MB(9) }
#undef HISEG_MB
  return hiseg_check_launch("morph_bilateral");
}

extern "C" int hiseg_bilateral_fwd(const float* x, float* out, long long NC, int H, int W, int kernel_size,
                                   float sigma_spatial, float sigma_range, hiseg_stream_t stream) {
  HISEG_REQUIRE(good_k(kernel_size), HISEG_ERR_BAD_ARG, "bilateral: kernel_size %d (odd, 3..9)", kernel_size);
  HISEG_REQUIRE(sigma_spatial > 0.f && sigma_range > 0.f, HISEG_ERR_BAD_ARG, "bilateral: sigma %g %g",
                (double)sigma_spatial, (double)sigma_range);
  HISEG_REQUIRE(NC >= 0 && H >= 0 && W >= 0 && (long long)H * W <= 0x7fffffffll, HISEG_ERR_BAD_SHAPE,
                "bilateral: planes %lld H %d W %d", NC, H, W);
  if (NC == 0 || H == 0 || W == 0) return HISEG_OK;
  HISEG_REQUIRE(x && out, HISEG_ERR_BAD_ARG, "bilateral: null pointer");
  HISEG_REQUIRE(H > kernel_size / 2 && W > kernel_size / 2, HISEG_ERR_BAD_ARG,
                "bilateral: reflect padding %d needs H, W > %d (got %d x %d)", kernel_size / 2, kernel_size / 2, H, W);
  const long long HW = (long long)H * W;
  HISEG_REQUIRE(NC <= 0x7fffffffffffffffll / HW, HISEG_ERR_BAD_SHAPE, "bilateral: planes %lld", NC);
  const long long total = NC * HW;
  PostWeights wt;
  gaussian_weights(kernel_size, sigma_spatial, false, &wt);
  const float inv2sr = 1.f / (2.f * sigma_range * sigma_range);
  const long long blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < 65536 * 16 ? blocks : 65536 * 16));
  hipStream_t s = (hipStream_t)stream;
#define HISEG_BL(K)                                                                                            \
  case K:                                                                                                      \
    hipLaunchKernelGGL(bilateral_kernel<K>, grid, dim3(256), 0, s, x, out, total, H, W, wt, inv2sr);           \
    break;
  switch (kernel_size) { HISEG_BL(3) HISEG_BL(5) HISEG_BL(7) HISEG_BL(9) }
#undef HISEG_BL
  return hiseg_check_launch("bilateral");
}

// ---- EdgePreservingFilter (bilateral_filter.py:219-296): the guided filter
//
// out = box(a)*g + box(b), a = (box(x*g) - box(x)*box(g)) / (box(g*g) - box(g)^2 + eps), b = box(x) - a*box(g); box is
// the zero-padded k x k sum (k = 2r+1) divided by k*k.  One workgroup owns a tile of one output plane.  The inputs
// live in LDS on a halo of 2R around the tile, a and b on a halo of R; R = r in the tiled form and 0 in the
// resident form (the tile is the plane, and a tap outside it is the zero padding).  Every box is separable: row sums
// first, then column sums, each a plain f32 sum over dx (dy) = -r..r in that order.  A tap that is skipped because
// it lies outside the plane would have added an exact zero, so a pixel sees the same additions in the same order
// wherever its tile lies: both forms give the same bits.  a and b are zero outside the image, as the reference's
// second convolution pads them, also where their own window overlaps the image.
//
// LDS: x and g over the input region, two row-sum planes (input rows x a/b columns), two a/b-domain planes: six
// f32 planes in the resident form, kGuidedResidentPx = 160 KB / 24 B pixels.  The four first-stage boxes go through
// the two row-sum planes in two rounds (x and g, then x*g and g*g).

namespace hiseg {

constexpr int kGuidedResidentPx = kPostLds / 24;
constexpr int kGuidedMaxRadius = kMaxHalo / 2;

struct GuidedGeom {
  int H, W;            // plane
  int TH, TW;          // tile
  int tiles_x, tiles;  // tiles per row / per plane
  int R;               // halo of a and b around the tile; the inputs carry 2R
  int Cx, Cg, Co;      // channels of x, of the guide and of out (the broadcast of the two)
};

// d1[row][c] = sum over dx = -r..r of s1[row][c + off + dx] (d2 of s2 likewise), rows x DW from rows x SW; PROD:
// of s1*s2 and s2*s2.  Taps outside the source row are zero padding and add nothing.
template <bool PROD>
__device__ __forceinline__ void row_sums(const float* s1, const float* s2, float* d1, float* d2, int rows, int SW,
                                         int DW, int off, int r) {
  for (int i = threadIdx.x; i < rows * DW; i += blockDim.x) {
    const int row = i / DW, c = i - row * DW;
    const int lo = max(c + off - r, 0), hi = min(c + off + r, SW - 1);
    const float* p1 = s1 + row * SW;
    const float* p2 = s2 + row * SW;
    float u = 0.f, v = 0.f;
    for (int k = lo; k <= hi; ++k) {
      const float e1 = p1[k], e2 = p2[k];
      if constexpr (PROD) {
        u = fmaf(e1, e2, u);
        v = fmaf(e2, e2, v);
      } else {
        u += e1;
        v += e2;
      }
    }
    d1[i] = u;
    d2[i] = v;
  }
  __syncthreads();
}

// Sum over dy = -r..r of s[row + dy][col] in a plane of SH x SW; rows outside it are zero padding.
__device__ __forceinline__ float col_sum(const float* s, int SH, int SW, int row, int col, int r) {
  const int lo = max(row - r, 0), hi = min(row + r, SH - 1);
  float u = 0.f;
  for (int k = lo; k <= hi; ++k) u += s[k * SW + col];
  return u;
}

__global__ void __launch_bounds__(1024) guided_filter_kernel(const float* __restrict__ x, const float* __restrict__ guide,
                                                             float* __restrict__ out, GuidedGeom q, int r, float eps) {
  extern __shared__ float post_lds[];
  const long long plane = blockIdx.x / q.tiles;
  const int tile = (int)(blockIdx.x % q.tiles);
  const int ty0 = (tile / q.tiles_x) * q.TH, tx0 = (tile % q.tiles_x) * q.TW;
  const int RH = q.TH + 4 * q.R, RW = q.TW + 4 * q.R;   // input region
  const int AH = q.TH + 2 * q.R, AW = q.TW + 2 * q.R;   // a / b domain
  const long long HW = (long long)q.H * q.W;
  const float kk = (float)((2 * r + 1) * (2 * r + 1));
  float* X = post_lds;
  float* G = X + RH * RW;
  float* h1 = G + RH * RW;      // row sums: RH x AW (the last stage uses AH x TW of it)
  float* h2 = h1 + RH * AW;
  float* m1 = h2 + RH * AW;     // AH x AW: box(x) then a
  float* m2 = m1 + AH * AW;     //          box(g) then b

  const long long bi = plane / q.Co;
  const int c = (int)(plane % q.Co);
  const float* xs = x + (bi * q.Cx + (q.Cx == 1 ? 0 : c)) * HW;
  const float* gs = guide + (bi * q.Cg + (q.Cg == 1 ? 0 : c)) * HW;
  for (int i = threadIdx.x; i < RH * RW; i += blockDim.x) {
    const int ly = i / RW, lx = i - ly * RW;
    const int gy = ty0 - 2 * q.R + ly, gx = tx0 - 2 * q.R + lx;
    float vx = 0.f, vg = 0.f;
    if ((unsigned)gy < (unsigned)q.H && (unsigned)gx < (unsigned)q.W) {
      const long long px = (long long)gy * q.W + gx;
      vx = xs[px];
      vg = gs[px];
    }
    X[i] = vx;
    G[i] = vg;
  }
  __syncthreads();

  row_sums<false>(X, G, h1, h2, RH, RW, AW, q.R, r);
  for (int i = threadIdx.x; i < AH * AW; i += blockDim.x) {
    const int ra = i / AW, ca = i - ra * AW;
    m1[i] = col_sum(h1, RH, AW, ra + q.R, ca, r) / kk;
    m2[i] = col_sum(h2, RH, AW, ra + q.R, ca, r) / kk;
  }
  __syncthreads();
  row_sums<true>(X, G, h1, h2, RH, RW, AW, q.R, r);
  for (int i = threadIdx.x; i < AH * AW; i += blockDim.x) {
    const int ra = i / AW, ca = i - ra * AW;
    const int gy = ty0 - q.R + ra, gx = tx0 - q.R + ca;
    float a = 0.f, b = 0.f;
    if ((unsigned)gy < (unsigned)q.H && (unsigned)gx < (unsigned)q.W) {
      const float mean_x = m1[i], mean_g = m2[i];
      const float corr_xg = col_sum(h1, RH, AW, ra + q.R, ca, r) / kk;
      const float corr_gg = col_sum(h2, RH, AW, ra + q.R, ca, r) / kk;
      a = (corr_xg - mean_x * mean_g) / (corr_gg - mean_g * mean_g + eps);
      b = mean_x - a * mean_g;
    }
    m1[i] = a;
    m2[i] = b;
  }
  __syncthreads();
  row_sums<false>(m1, m2, h1, h2, AH, AW, q.TW, q.R, r);
  float* dst = out + plane * HW;
  for (int i = threadIdx.x; i < q.TH * q.TW; i += blockDim.x) {
    const int ty = i / q.TW, tx = i - ty * q.TW;
    const int gy = ty0 + ty, gx = tx0 + tx;
    if (gy < q.H && gx < q.W) {
      const float mean_a = col_sum(h1, AH, q.TW, ty + q.R, tx, r) / kk;
      const float mean_b = col_sum(h2, AH, q.TW, ty + q.R, tx, r) / kk;
      dst[(long long)gy * q.W + gx] = mean_a * G[(ty + 2 * q.R) * RW + tx + 2 * q.R] + mean_b;
    }
  }
}

// f32 words of LDS of one workgroup.
static long long guided_lds_words(int TH, int TW, int R) {
  const long long RH = TH + 4 * R, RW = TW + 4 * R, AH = TH + 2 * R, AW = TW + 2 * R;
  return 2 * RH * RW + 2 * RH * AW + 2 * AH * AW;
}

// Rows of a tile of the tiled form: 64 up to radius 6, then the largest of 32, 16, 8 whose working set fits the
// LDS (32 up to radius 11, 16 up to 14, 8 for 15 and 16).  The tile stays 64 columns wide.
static int guided_tile_rows(int radius) {
  for (int th = kPostTile; th >= 8; th /= 2)
    if (guided_lds_words(th, kPostTile, radius) * 4 <= kPostLds) return th;
  return 0;
}

}  // namespace hiseg

extern "C" int hiseg_guided_filter_fwd(const float* x, const float* guide, float* out, long long B, int Cx, int Cg,
                                       int H, int W, int radius, float eps, int force_tiled, hiseg_stream_t stream) {
  HISEG_REQUIRE(radius >= 1 && radius <= kGuidedMaxRadius, HISEG_ERR_BAD_ARG, "guided_filter: radius %d (1..%d)",
                radius, kGuidedMaxRadius);
  if (!guide) Cg = Cx;
  HISEG_REQUIRE(Cx >= 0 && Cg >= 0 && (Cx == Cg || Cx == 1 || Cg == 1), HISEG_ERR_BAD_ARG,
                "guided_filter: channels %d and %d do not broadcast", Cx, Cg);
  HISEG_REQUIRE(B >= 0 && H >= 0 && W >= 0 && (long long)H * W <= 0x7fffffffll, HISEG_ERR_BAD_SHAPE,
                "guided_filter: batch %lld H %d W %d", B, H, W);
  const int Co = Cx > Cg ? Cx : Cg;
  if (B == 0 || Cx == 0 || Cg == 0 || H == 0 || W == 0) return HISEG_OK;
  HISEG_REQUIRE(x && out, HISEG_ERR_BAD_ARG, "guided_filter: null pointer");
  HISEG_REQUIRE(out != x && out != guide, HISEG_ERR_BAD_ARG, "guided_filter: out aliases an input");
  GuidedGeom q;
  q.H = H; q.W = W; q.Cx = Cx; q.Cg = Cg; q.Co = Co;
  unsigned block;
  if (!force_tiled && (long long)H * W <= kGuidedResidentPx) {
    q.TH = H; q.TW = W; q.tiles_x = 1; q.tiles = 1; q.R = 0;
    block = H * W >= 1024 ? 1024u : (unsigned)((H * W + 63) / 64 * 64);
  } else {
    q.TH = guided_tile_rows(radius);
    HISEG_REQUIRE(q.TH > 0, HISEG_ERR_BAD_ARG, "guided_filter: radius %d does not fit the LDS", radius);
    q.TW = kPostTile;
    q.R = radius;
    q.tiles_x = (W + q.TW - 1) / q.TW;
    q.tiles = q.tiles_x * ((H + q.TH - 1) / q.TH);
    block = 1024;
  }
  HISEG_REQUIRE(B <= 0x7fffffffll / Co && B * Co <= 0x7fffffffll / q.tiles, HISEG_ERR_BAD_SHAPE,
                "guided_filter: %lld planes of %d tiles", B * Co, q.tiles);
  const size_t lds = (size_t)guided_lds_words(q.TH, q.TW, q.R) * sizeof(float);
  (void)hipFuncSetAttribute((const void*)guided_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kPostLds);
  hipLaunchKernelGGL(guided_filter_kernel, dim3((unsigned)(B * Co * q.tiles)), dim3(block), lds, (hipStream_t)stream,
                     x, guide ? guide : x, out, q, radius, eps);
  return hiseg_check_launch("guided_filter");
}

// ---- DirectionalEdgeSmoothing, AdaptiveEdgeSmoothing, OptimizedEdgeSmoothing (export_edge_smoothing_onnx.py)
//
// The kernel shape of edge_smooth_kernel with a stencil of radius 2: one stage per iteration reads buffer a and
// writes the 0/1 decision to buffer b, so the two-buffer budget (kResidentPx, kMaxHalo) is unchanged and the tiled
// halo is 2 * iterations.  The optimized filter's separable Gaussian is evaluated per output pixel as the vertical
// 5-tap sum of the five horizontal 5-tap sums it needs (25 LDS reads, the reference's two summations in their order)
// rather than through a third LDS plane.  LDS reads: lane l reads word base + l for every tap of a row stencil and
// base + l +- RW for the column taps, stride 1 over the 32 ds_read_b32 banks, conflict-free but for the row wrap.
// The pre-threshold blend of the last iteration goes to `soft` from the thread that computed it.  f16 planes are
// widened while the region is loaded and narrowed in the final store; everything between is f32.

namespace hiseg {

constexpr int kVarDir = 0, kVarAdaptive = 1, kVarOpt = 2;
constexpr int kVariantRadius = 2;

struct VariantParams {
  const float* blur_strength;     // adaptive only: device arrays, element plane * stride
  const float* edge_sensitivity;
  const float* final_threshold;
  long long stride;
};

__device__ __forceinline__ float load_px(const float* p) { return *p; }
__device__ __forceinline__ float load_px(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ void store_px(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_px(__half* p, float v) { *p = __float2half(v); }

// The 3x3 neighbourhood of (ly, lx) with zero padding; n[1][1] is the pixel.
struct Nbr3 { float n[3][3]; };
__device__ __forceinline__ Nbr3 nbr3(const Region& r, const float* a, int ly, int lx) {
  Nbr3 q;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) q.n[dy][dx] = r.tap(a, ly + dy - 1, lx + dx - 1, 0.f);
  }
  return q;
}

__device__ __forceinline__ float laplacian8(const Nbr3& q) {
#pragma clang fp contract(off)
  return 8.f * q.n[1][1] - (((q.n[0][0] + q.n[0][1]) + (q.n[0][2] + q.n[1][0])) +
                            ((q.n[1][2] + q.n[2][0]) + (q.n[2][1] + q.n[2][2])));
}

// DirectionalEdgeSmoothing.forward (:114-150) before the threshold.  IEEE f32 libm and divisions, every product
// and sum rounded on its own in the reference's order.
__device__ __forceinline__ float dir_blend(const Region& r, const float* a, int ly, int lx) {
#pragma clang fp contract(off)
  const Nbr3 q = nbr3(r, a, ly, lx);
  const float c = q.n[1][1];
  const float l2 = r.tap(a, ly, lx - 2, 0.f), r2 = r.tap(a, ly, lx + 2, 0.f);
  const float u2 = r.tap(a, ly - 2, lx, 0.f), d2 = r.tap(a, ly + 2, lx, 0.f);
  const float ex = ((((q.n[0][2] - q.n[0][0]) - 2.f * q.n[1][0]) + 2.f * q.n[1][2]) - q.n[2][0]) + q.n[2][2];
  const float ey = ((((-q.n[0][0] - 2.f * q.n[0][1]) - q.n[0][2]) + q.n[2][0]) + 2.f * q.n[2][1]) + q.n[2][2];
  const float mag = sqrtf((ex * ex + ey * ey) + 1e-8f);
  const float ang = atan2f(ey, ex);
  const float bh = (((0.1f * l2 + 0.2f * q.n[1][0]) + 0.4f * c) + 0.2f * q.n[1][2]) + 0.1f * r2;
  const float bv = (((0.1f * u2 + 0.2f * q.n[0][1]) + 0.4f * c) + 0.2f * q.n[2][1]) + 0.1f * d2;
  const float bd1 = (0.1f * q.n[0][0] + 0.8f * c) + 0.1f * q.n[2][2];
  const float bd2 = (0.1f * q.n[0][2] + 0.8f * c) + 0.1f * q.n[2][0];
  const float kQuarterPi = 0.78539816339744830962f;
  const float ch = cosf(ang), sh = sinf(ang), c1 = cosf(ang - kQuarterPi), c2 = cosf(ang + kQuarterPi);
  float wh = ch * ch, wv = sh * sh, wd1 = (c1 * c1) * 0.5f, wd2 = (c2 * c2) * 0.5f;
  const float ws = (((wh + wv) + wd1) + wd2) + 1e-8f;
  wh = wh / ws;
  wv = wv / ws;
  wd1 = wd1 / ws;
  wd2 = wd2 / ws;
  const float blurred = ((bh * wh + bv * wv) + bd1 * wd1) + bd2 * wd2;
  return blend_f32(c, blurred, sigmoid_f32(mag * 3.0f));
}

// AdaptiveEdgeSmoothing.forward (:183-208) before the threshold; half_es = 0.5 * edge_sensitivity,
// bf = blur_strength / 3.
__device__ __forceinline__ float adaptive_blend(const Region& r, const float* a, int ly, int lx, float half_es,
                                                float bf) {
#pragma clang fp contract(off)
  const Nbr3 q = nbr3(r, a, ly, lx);
  const float c = q.n[1][1];
  const float edge = fabsf(laplacian8(q)) > half_es ? 1.f : 0.f;
  float mean = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const float v = (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) ? q.n[dy + 1][dx + 1] : r.tap(a, ly + dy, lx + dx, 0.f);
      mean = mean + 0.04f * v;
    }
  }
  const float smoothed = blend_f32(c, mean, bf);
  return blend_f32(c, smoothed, edge);
}

// OptimizedEdgeSmoothing.forward (:293-310) before the threshold.
__device__ __forceinline__ float opt_blend(const Region& r, const float* a, int ly, int lx) {
#pragma clang fp contract(off)
  const float w[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  float rows[5][5];
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) rows[dy][dx] = r.tap(a, ly + dy - 2, lx + dx - 2, 0.f);
  }
  Nbr3 q;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) q.n[dy][dx] = rows[dy + 1][dx + 1];
  }
  float blurred = 0.f;
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    float h = 0.f;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) h = h + w[dx] * rows[dy][dx];
    blurred = blurred + w[dy] * h;
  }
  const float scaled = fabsf(laplacian8(q)) * 3.0f;
  const float e = fminf(fmaxf((scaled + 0.5f) * 0.5f, 0.f), 1.f);
  return blend_f32(q.n[1][1], blurred, e);
}

// TI / TO: the types of the planes x and out.  f32 in with f16 out rounds x to f16 while it is loaded: the f16 path
// on an f32 mask (OptimizedEdgeSmoothing(use_fp16=True) behind the wrapper's f32 masks) without a cast pass.
template <int KIND, typename TI, typename TO>
__global__ void __launch_bounds__(1024) edge_variant_kernel(const TI* __restrict__ x, TO* __restrict__ out,
                                                            float* __restrict__ soft, PostGeom g, VariantParams vp,
                                                            int iterations) {
  extern __shared__ float post_lds[];
  const long long plane = blockIdx.x / g.tiles;
  const Region r = region_of(g, (int)(blockIdx.x % g.tiles));
  const long long HW = (long long)g.H * g.W;
  const int n = r.size();
  float* a = post_lds;
  float* b = post_lds + n;

  float thr = 0.5f, half_es = 0.f, bf = 0.f;
  if constexpr (KIND == kVarAdaptive) {
    const long long pi = plane * vp.stride;
    thr = vp.final_threshold[pi];
    half_es = 0.5f * vp.edge_sensitivity[pi];
    bf = vp.blur_strength[pi] / 3.0f;
  }

  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ly = i / r.RW, lx = i - ly * r.RW;
    float v = 0.f;
    if (r.in_image(ly, lx)) {
      v = load_px(x + plane * HW + (long long)(r.y0 + ly) * g.W + (r.x0 + lx));
      if constexpr (sizeof(TI) > sizeof(TO)) v = __half2float(__float2half(v));
    }
    a[i] = v;
  }
  __syncthreads();

  for (int it = 0; it < iterations; ++it) {
    const bool want_soft = soft != nullptr && it == iterations - 1;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int ly = i / r.RW, lx = i - ly * r.RW;
      float o = 0.f;
      if (r.in_image(ly, lx)) {
        float v;
        if constexpr (KIND == kVarDir) v = dir_blend(r, a, ly, lx);
        else if constexpr (KIND == kVarAdaptive) v = adaptive_blend(r, a, ly, lx, half_es, bf);
        else v = opt_blend(r, a, ly, lx);
        o = v > thr ? 1.f : 0.f;
        if (want_soft && ly >= g.R && ly < g.R + g.TH && lx >= g.R && lx < g.R + g.TW)
          soft[plane * HW + (long long)(r.y0 + ly) * g.W + (r.x0 + lx)] = v;
      }
      b[i] = o;
    }
    __syncthreads();
    float* t = a; a = b; b = t;
  }
  TO* dst = out + plane * HW;
  for (int i = threadIdx.x; i < g.TH * g.TW; i += blockDim.x) {
    const int ty = i / g.TW, tx = i - ty * g.TW;
    const int gy = r.y0 + g.R + ty, gx = r.x0 + g.R + tx;
    if (gy < g.H && gx < g.W) store_px(dst + (long long)gy * g.W + gx, a[(ty + g.R) * r.RW + tx + g.R]);
  }
}

}  // namespace hiseg

namespace {

template <int KIND, typename TI, typename TO>
int edge_variant(const char* what, const TI* x, TO* out, float* soft, long long NC, int H, int W,
                 const VariantParams& vp, int iterations, int force_tiled, hiseg_stream_t stream) {
  HISEG_REQUIRE(iterations >= 1, HISEG_ERR_BAD_ARG, "%s: iterations %d", what, iterations);
  PostPlan p;
  const long long halo = (long long)iterations * kVariantRadius;
  const int st = post_plan(what, x, out, NC, H, W, halo > kMaxHalo ? kMaxHalo + 1 : (int)halo, force_tiled, &p);
  if (st != HISEG_OK || p.grid == 0) return st;
  HISEG_REQUIRE((const void*)x != (const void*)out && (const void*)soft != (const void*)x &&
                    (const void*)soft != (const void*)out,
                HISEG_ERR_BAD_ARG, "%s: x, out and soft alias", what);
  if constexpr (KIND == kVarAdaptive) {
    HISEG_REQUIRE(vp.blur_strength && vp.edge_sensitivity && vp.final_threshold && vp.stride >= 0, HISEG_ERR_BAD_ARG,
                  "%s: null parameter array or negative param_stride %lld", what, vp.stride);
  }
  post_launch(edge_variant_kernel<KIND, TI, TO>, p, (hipStream_t)stream, x, out, soft, p.g, vp, iterations);
  return hiseg_check_launch(what);
}

}  // namespace

extern "C" int hiseg_dir_edge_smooth_fwd(const float* x, float* out, float* soft, long long NC, int H, int W,
                                         int iterations, int force_tiled, hiseg_stream_t stream) {
  return edge_variant<kVarDir, float, float>("dir_edge_smooth", x, out, soft, NC, H, W, VariantParams{}, iterations,
                                      force_tiled, stream);
}

extern "C" int hiseg_adaptive_edge_smooth_fwd(const float* x, float* out, float* soft, long long NC, int H, int W,
                                              const float* blur_strength, const float* edge_sensitivity,
                                              const float* final_threshold, long long param_stride, int iterations,
                                              int force_tiled, hiseg_stream_t stream) {
  const VariantParams vp{blur_strength, edge_sensitivity, final_threshold, param_stride};
  return edge_variant<kVarAdaptive, float, float>("adaptive_edge_smooth", x, out, soft, NC, H, W, vp, iterations,
                                           force_tiled, stream);
}

extern "C" int hiseg_opt_edge_smooth_fwd(int dtype, const void* x, void* out, float* soft, long long NC, int H, int W,
                                         int iterations, int force_tiled, hiseg_stream_t stream) {
  if (dtype == HISEG_POST_F16)
    return edge_variant<kVarOpt, __half, __half>("opt_edge_smooth", (const __half*)x, (__half*)out, soft, NC, H, W,
                                                 VariantParams{}, iterations, force_tiled, stream);
  if (dtype == HISEG_POST_F32_TO_F16)
    return edge_variant<kVarOpt, float, __half>("opt_edge_smooth", (const float*)x, (__half*)out, soft, NC, H, W,
                                                VariantParams{}, iterations, force_tiled, stream);
  HISEG_REQUIRE(dtype == HISEG_POST_F32, HISEG_ERR_BAD_DTYPE, "opt_edge_smooth: dtype %d (f32 or f16 planes)", dtype);
  return edge_variant<kVarOpt, float, float>("opt_edge_smooth", (const float*)x, (float*)out, soft, NC, H, W,
                                      VariantParams{}, iterations, force_tiled, stream);
}
