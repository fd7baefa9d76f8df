// Full-frame instance composition (include/hiseg_compose.h): per-ROI masks -> bit-packed masks + scores, packed
// masks + boxes -> one label map per frame, label map + image -> colour overlay.  All three are byte-stream passes
// (HBM / L2 bound).  Nothing here uses an atomic: the ROI front end owns a ROI per workgroup and reduces through a
// fixed tree, the frame passes write every output element exactly once.
#include <math.h>

#include "common.h"
#include "hiseg_compose.h"

namespace hiseg {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileW = 128, kTileH = 8;   // 32 lanes x 4 pixels per row, 8 rows: 1024 labels per workgroup
constexpr int kRoiChunk = 64;             // ROIs tested per pass: one wave, one ballot

// ---------------------------------------------------------------------------------------------- ROI front end
// One workgroup per ROI walks the padded positions p = row * wpr * 32 + col in steps of 256: a wave covers 64
// consecutive positions = two whole words of one row or of two adjacent rows, so its ballot IS the packed output.
template <bool kLogits>
__global__ void __launch_bounds__(kThreads) roi_bits_kernel(const float* __restrict__ src, int mh, int mw, int wpr,
                                                            float thr, unsigned int* __restrict__ bits,
                                                            float* __restrict__ score, int* __restrict__ count) {
  const long long n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hw = mh * mw, rowpos = wpr * 32;
  const int words = mh * wpr;                     // (checked on the host: mh * wpr * 32 fits an int)
  const float* x = src + n * (kLogits ? 3 : 1) * (long long)hw;
  unsigned int* o = bits + n * (long long)words;
  float sum = 0.f;
  int cnt = 0;
  for (int base = 0; base < words * 32; base += kThreads) {
    const int p = base + threadIdx.x;
    const int row = p / rowpos, col = p - row * rowpos;
    bool set = false;
    float pmax = 0.f;
    if (row < mh && col < mw) {
      const int i = row * mw + col;
      if constexpr (kLogits) {
        const float l0 = x[i], l1 = x[hw + i], l2 = x[2 * hw + i];
        const float m = fmaxf(l0, fmaxf(l1, l2));
        const float s = __fadd_rn(__fadd_rn(expf(l0 - m), expf(l1 - m)), expf(l2 - m));
        pmax = 1.0f / s;                          // exp(max - max) / sum
        set = l1 > l0 && !(l2 > l1) && pmax > thr;   // first maximum is class 1
      } else {
        set = x[i] > 0.5f;
      }
    }
    const unsigned long long b = __ballot(set);
    const int w = (base >> 5) + wave * 2;         // this wave's first word
    if (lane == 0 && w < words) o[w] = (unsigned int)b;
    if (lane == 32 && w + 1 < words) o[w + 1] = (unsigned int)(b >> 32);
    if (set) {
      sum += pmax;
      ++cnt;
    }
  }
  // fixed tree: 64 lanes by shuffles, then the four waves in order
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sum += __shfl_xor(sum, d, 64);
    cnt += __shfl_xor(cnt, d, 64);
  }
  __shared__ float s_sum[kWaves];
  __shared__ int s_cnt[kWaves];
  if (lane == 0) {
    s_sum[wave] = sum;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    count[n] = c;
    score[n] = kLogits ? (c > 0 ? t / (float)c : 0.f) : (c > 0 ? 1.f : 0.f);
  }
}

// ---------------------------------------------------------------------------------------------- label map
// int(v) of denormalize_bbox for an f32 product; false for a NaN
__device__ __forceinline__ bool box_px(float norm, int size, int* out) {
  const float v = __fmul_rn(norm, (float)size);
  if (!(v == v)) return false;
  *out = (int)fminf(fmaxf(v, -1e9f), 1e9f);
  return true;
}

// cv2.resize(..., INTER_NEAREST) source index (OpenCV resizeNN), with ifx = 1.0 / (dst / (double)src)
__device__ __forceinline__ int nn_src(int x, double ifx, int src) {
  const int s = (int)floor((double)x * ifx);
  return s < src - 1 ? s : src - 1;
}

template <bool kVec>
__global__ void __launch_bounds__(kThreads) instance_map_kernel(const unsigned int* __restrict__ bits,
                                                                const float* __restrict__ score,
                                                                const float* __restrict__ rois, long long N, int mh,
                                                                int mw, int wpr, int H, int W,
                                                                int* __restrict__ label) {
  __shared__ int s_x1[kRoiChunk], s_y1[kRoiChunk], s_x2[kRoiChunk], s_y2[kRoiChunk];
  __shared__ double s_ifx[kRoiChunk], s_ify[kRoiChunk];
  __shared__ long long s_k[kRoiChunk];
  __shared__ int s_n;
  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int tx1 = min(tx0 + kTileW, W), ty1 = min(ty0 + kTileH, H);
  const int px = tx0 + (threadIdx.x & 31) * 4, py = ty0 + (threadIdx.x >> 5);
  const bool live = py < H && px < W;
  int own[4] = {0, 0, 0, 0};
  // pixels of this thread outside the frame count as owned: they are never written and must not hold the tile back
  int open = 0;
  if (live) open = min(4, W - px);

  for (long long base = N > 0 ? (N - 1) / kRoiChunk * kRoiChunk : -1; base >= 0; base -= kRoiChunk) {
    if (threadIdx.x < 64) {   // wave 0 tests one ROI per lane and compacts the survivors in index order
      const long long k = base + threadIdx.x;
      bool keep = false;
      int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
      if (k < N) {
        const float* r = rois + k * 5;
        keep = r[0] == (float)b && score[k] > 0.f && box_px(r[1], W, &x1) && box_px(r[2], H, &y1) &&
               box_px(r[3], W, &x2) && box_px(r[4], H, &y2);
        keep = keep && x2 > x1 && y2 > y1 && x1 < tx1 && x2 > tx0 && y1 < ty1 && y2 > ty0;
      }
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int pos = __popcll(m & ((1ull << threadIdx.x) - 1ull));
        s_x1[pos] = x1; s_y1[pos] = y1; s_x2[pos] = x2; s_y2[pos] = y2;
        s_ifx[pos] = 1.0 / ((double)(x2 - x1) / (double)mw);
        s_ify[pos] = 1.0 / ((double)(y2 - y1) / (double)mh);
        s_k[pos] = k;
      }
      if (threadIdx.x == 0) s_n = __popcll(m);
    }
    __syncthreads();
    const int n = s_n;
    for (int e = n - 1; e >= 0 && open > 0; --e) {
      const int y1 = s_y1[e];
      if (py < y1 || py >= s_y2[e]) continue;
      const int x1 = s_x1[e], x2 = s_x2[e];
      if (px + 3 < x1 || px >= x2) continue;
      const int sy = nn_src(py - y1, s_ify[e], mh);
      const unsigned int* row = bits + (s_k[e] * mh + sy) * (long long)wpr;
      const double ifx = s_ifx[e];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x = px + i;
        if (own[i] == 0 && x >= x1 && x < x2 && x < W) {
          const int sx = nn_src(x - x1, ifx, mw);
          if ((row[sx >> 5] >> (sx & 31)) & 1u) {
            own[i] = (int)s_k[e] + 1;
            --open;
          }
        }
      }
    }
    if (__syncthreads_and(open == 0)) break;   // (also the barrier before the next chunk overwrites the list)
  }

  if (!live) return;
  int* o = label + ((long long)b * H + py) * W + px;
  if (kVec) {                 // W % 4 == 0: px + 3 < W and the address is 16-byte aligned
    *reinterpret_cast<int4*>(o) = make_int4(own[0], own[1], own[2], own[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (px + i < W) o[i] = own[i];
  }
}

// ---------------------------------------------------------------------------------------------- overlay
__device__ __forceinline__ unsigned int blend8(unsigned int img, unsigned int col, float wi, float wo) {
  const float v = rintf(__fadd_rn(__fmul_rn((float)img, wi), __fmul_rn((float)col, wo)));   // half to even
  return (unsigned int)fminf(fmaxf(v, 0.f), 255.f);
}

// One thread per 4 pixels of the flat [B*H*W] range: 16 B of labels, 12 B of image in, 12 B out (three words).
__global__ void __launch_bounds__(kThreads) overlay_kernel(const int* __restrict__ label,
                                                           const unsigned char* __restrict__ image,
                                                           const unsigned char* __restrict__ colors, long long N,
                                                           long long P, float wi, float wo,
                                                           unsigned char* __restrict__ out) {
  const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (p0 >= P) return;
  if (p0 + 4 <= P) {
    const int4 l4 = *reinterpret_cast<const int4*>(label + p0);
    const int l[4] = {l4.x, l4.y, l4.z, l4.w};
    const unsigned int* in = reinterpret_cast<const unsigned int*>(image + p0 * 3);
    const unsigned int w[3] = {in[0], in[1], in[2]};
    unsigned int r[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool has = l[i] > 0 && l[i] <= N;
      const unsigned char* c = colors + (has ? (long long)(l[i] - 1) * 3 : 0);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int byte = i * 3 + ch;
        const unsigned int img = (w[byte >> 2] >> ((byte & 3) * 8)) & 0xffu;
        const unsigned int col = has ? (unsigned int)c[ch] : 0u;
        r[byte >> 2] |= blend8(img, col, wi, wo) << ((byte & 3) * 8);
      }
    }
    unsigned int* o = reinterpret_cast<unsigned int*>(out + p0 * 3);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
  } else {                    // the last, partial group
    for (long long p = p0; p < P; ++p) {
      const int l = label[p];
      const bool has = l > 0 && l <= N;
      for (int ch = 0; ch < 3; ++ch) {
        const unsigned int col = has ? (unsigned int)colors[(long long)(l - 1) * 3 + ch] : 0u;
        out[p * 3 + ch] = (unsigned char)blend8(image[p * 3 + ch], col, wi, wo);
      }
    }
  }
}

}  // namespace hiseg

using namespace hiseg;

extern "C" int hiseg_compose_words_per_row(int mw) { return mw > 0 ? (mw + 31) / 32 : 0; }

static int roi_bits_launch(const char* what, bool logits, const float* src, long long N, int mh, int mw, float thr,
                           unsigned int* bits, float* score, int* count, hiseg_stream_t stream) {
  HISEG_REQUIRE(N >= 0, HISEG_ERR_BAD_ARG, "%s: negative N (%lld)", what, N);
  HISEG_REQUIRE(mh > 0 && mw > 0, HISEG_ERR_BAD_ARG, "%s: mh*mw == 0 or negative (mh %d, mw %d)", what, mh, mw);
  const long long wpr = hiseg_compose_words_per_row(mw);
  HISEG_REQUIRE((long long)mh * wpr * 32 < (1ll << 31) && (long long)mh * mw * 3 < (1ll << 31), HISEG_ERR_BAD_SHAPE,
                "%s: mask %d x %d too large", what, mh, mw);
  HISEG_REQUIRE(N < (1ll << 31), HISEG_ERR_BAD_SHAPE, "%s: N %lld too large", what, N);
  if (N == 0) return HISEG_OK;
  HISEG_REQUIRE(src && bits && score && count, HISEG_ERR_BAD_ARG, "%s: null pointer", what);
  if (logits)
    hipLaunchKernelGGL(roi_bits_kernel<true>, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, src, mh, mw,
                       (int)wpr, thr, bits, score, count);
  else
    hipLaunchKernelGGL(roi_bits_kernel<false>, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, src, mh, mw,
                       (int)wpr, thr, bits, score, count);
  return hiseg_check_launch(what);
}

extern "C" int hiseg_roi_mask_classify_fwd(const float* logits, long long N, int mh, int mw, float score_threshold,
                                           unsigned int* bits, float* score, int* count, hiseg_stream_t stream) {
  return roi_bits_launch("roi_mask_classify", true, logits, N, mh, mw, score_threshold, bits, score, count, stream);
}

extern "C" int hiseg_roi_mask_pack_fwd(const float* masks, long long N, int mh, int mw, unsigned int* bits,
                                       float* score, int* count, hiseg_stream_t stream) {
  return roi_bits_launch("roi_mask_pack", false, masks, N, mh, mw, 0.5f, bits, score, count, stream);
}

extern "C" int hiseg_instance_map_fwd(const unsigned int* bits, const float* score, const float* rois, long long N,
                                      int mh, int mw, int B, int H, int W, int* label, hiseg_stream_t stream) {
  HISEG_REQUIRE(N >= 0, HISEG_ERR_BAD_ARG, "instance_map: negative N (%lld)", N);
  HISEG_REQUIRE(B >= 0 && H >= 0 && W >= 0, HISEG_ERR_BAD_ARG, "instance_map: negative frame size (%d, %d, %d)", B, H,
                W);
  HISEG_REQUIRE(mh > 0 && mw > 0, HISEG_ERR_BAD_ARG, "instance_map: mh*mw == 0 or negative (mh %d, mw %d)", mh, mw);
  HISEG_REQUIRE(N < (1ll << 31) - 1, HISEG_ERR_BAD_SHAPE, "instance_map: N %lld does not fit an i32 label", N);
  HISEG_REQUIRE(H < (1 << 24) && W < (1 << 24), HISEG_ERR_BAD_SHAPE, "instance_map: frame %d x %d too large", H, W);
  if ((long long)B * H * W == 0) return HISEG_OK;
  HISEG_REQUIRE(label, HISEG_ERR_BAD_ARG, "instance_map: null pointer (label)");
  HISEG_REQUIRE(N == 0 || (bits && score && rois), HISEG_ERR_BAD_ARG, "instance_map: null pointer");
  const unsigned gx = (unsigned)((W + kTileW - 1) / kTileW), gy = (unsigned)((H + kTileH - 1) / kTileH);
  HISEG_REQUIRE(gy <= 65535u && B <= 65535, HISEG_ERR_BAD_SHAPE, "instance_map: grid (%d frames, %d rows)", B, H);
  const int wpr = hiseg_compose_words_per_row(mw);
  const dim3 g(gx, gy, (unsigned)B);
  if (W % 4 == 0 && (reinterpret_cast<uintptr_t>(label) & 15) == 0)
    hipLaunchKernelGGL(instance_map_kernel<true>, g, dim3(kThreads), 0, (hipStream_t)stream, bits, score, rois, N, mh,
                       mw, wpr, H, W, label);
  else
    hipLaunchKernelGGL(instance_map_kernel<false>, g, dim3(kThreads), 0, (hipStream_t)stream, bits, score, rois, N, mh,
                       mw, wpr, H, W, label);
  return hiseg_check_launch("instance_map");
}

extern "C" int hiseg_instance_overlay_fwd(const int* label, const unsigned char* image, const unsigned char* colors,
                                          long long N, int B, int H, int W, double alpha, unsigned char* out,
                                          hiseg_stream_t stream) {
  HISEG_REQUIRE(N >= 0, HISEG_ERR_BAD_ARG, "instance_overlay: negative N (%lld)", N);
  HISEG_REQUIRE(B >= 0 && H >= 0 && W >= 0, HISEG_ERR_BAD_ARG, "instance_overlay: negative frame size (%d, %d, %d)",
                B, H, W);
  const long long P = (long long)B * H * W;
  if (P == 0) return HISEG_OK;
  HISEG_REQUIRE(label && image && out && (N == 0 || colors), HISEG_ERR_BAD_ARG, "instance_overlay: null pointer");
  HISEG_REQUIRE(image != out, HISEG_ERR_BAD_ARG, "instance_overlay: image and out alias");
  HISEG_REQUIRE(((reinterpret_cast<uintptr_t>(label) & 15) | (reinterpret_cast<uintptr_t>(image) & 3) |
                 (reinterpret_cast<uintptr_t>(out) & 3)) == 0,
                HISEG_ERR_BAD_ARG, "instance_overlay: label must be 16-byte aligned, image and out 4-byte aligned");
  const long long groups = (P + 3) / 4, blocks = (groups + kThreads - 1) / kThreads;
  HISEG_REQUIRE(blocks < (1ll << 31), HISEG_ERR_BAD_SHAPE, "instance_overlay: %lld pixels", P);
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, label, image,
                     colors, N, P, (float)(1.0 - alpha), (float)alpha, out);
  return hiseg_check_launch("instance_overlay");
}
