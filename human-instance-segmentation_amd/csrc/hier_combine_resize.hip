// Hierarchical combine at a mask size other than 2 x ROI (refinement.py:559-596, unet.py:785-836): the reference
// computes upsample_bg_fg and the target branch at 2h x 2w, resizes both bilinearly (align_corners=False) to
// (mh, mw), then takes the softmax and combines.  One launch does all of it: a workgroup owns a tile of mask pixels
// of one ROI, evaluates the upsample_bg_fg micro-network (ConvTranspose 2 -> 32 k2 s2, norm, act, 1x1 32 -> 2; the
// arithmetic of hier_combine_kernel, misc.hip) ONCE per pixel of the tile's source window of the 2h x 2w grid into
// LDS, next to the window's two target logits, and every mask pixel interpolates its four taps from there.  The
// bg/fg logits never exist at 2h x 2w in memory.
//
// Tile shapes (256 threads, one mask pixel each): 4 x 64 for wide masks, so that a wave stores one contiguous 256-B
// row segment per output plane (NCHW f32 rows of any width mw: consecutive lanes, consecutive addresses -- a mask row
// is not a multiple of 16 B in general, so the stores are 4 B per lane, coalesced over the wave), 8 x 32 and
// 16 x 16 for narrower masks (fewer idle lanes).  The window is 16 B per source pixel (b0, b1, t0, t1: one
// ds_read_b128 per tap); at the reference's largest ratio (mask = ROI, scale 2) a 4 x 64 tile is given 10 x 130
// pixels = 20 KiB, so seven workgroups fit the 160-KiB LDS of a compute unit.  The entry point refuses a ratio whose
// window would pass 48 KiB.
#include "common.h"

namespace hiseg {

// float4 entries: 48 KiB (with the 1.5 KiB of tables under the 64 KiB a workgroup gets)
constexpr int kCrWindowMax = 3072;

// Source index pair and weight of output index o (F.interpolate bilinear, align_corners=False: the arithmetic of
// resize_bilinear_kernel, misc.hip).  Plain operators with contraction off: a fused multiply-add moves the
// coordinate by an ulp, and with it the tap pair at an integer boundary (DESIGN Appendix A, round 4, item (2)).
__device__ __forceinline__ void cr_src(int o, float scale, int in, int& i0, int& i1, float& l) {
#pragma clang fp contract(off)
  float s = ((float)o + 0.5f) * scale;
  s = s - 0.5f;
  s = s < 0.f ? 0.f : s;
  int a = (int)s;
  a = a > in - 1 ? in - 1 : a;
  i0 = a;
  i1 = a + (a < in - 1 ? 1 : 0);
  l = s - (float)a;
}

__global__ void __launch_bounds__(256) hier_combine_resize_kernel(
    const float* low, int h, int w, const float* tn2, const float* ut_w, const float* ut_scale, const float* ut_shift,
    int ut_act, float ut_beta, int ut_ns, const float* u1_w, const float* u1_b, int mh, int mw, int tw_log2,
    int tiles_x, int tiles_y, int win_cap, float* logits, float* bgfg, float* tn) {
  extern __shared__ float4 s_win[];   // [rows][cols] of the source window: (b0, b1, t0, t1)
  __shared__ float s_ut[2 * 32 * 4], s_us[32], s_ush[32], s_u1[64];
  const int t = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int TW = 1 << tw_log2, TH = 256 >> tw_log2;
  const int oy0 = (tile / tiles_x) * TH, ox0 = (tile % tiles_x) * TW;
  const int H = 2 * h, W = 2 * w;
  s_ut[t] = ut_w[t];
  if (t < 32) {   // per-sample tables (LayerNorm2d: ut_ns == 32) are this ROI's row
    s_us[t] = ut_scale[(long long)n * ut_ns + t];
    s_ush[t] = ut_shift[(long long)n * ut_ns + t];
  }
  if (t < 64) s_u1[t] = u1_w[t];
  const float sh = (float)H / (float)mh, sw = (float)W / (float)mw;
  // the tile's source window: from the first tap of its first row / column to the second tap of its last
  const int oy1 = min(oy0 + TH, mh) - 1, ox1 = min(ox0 + TW, mw) - 1;
  int wy0, wy1, wx0, wx1, unused;
  float lu;
  cr_src(oy0, sh, H, wy0, unused, lu);
  cr_src(oy1, sh, H, unused, wy1, lu);
  cr_src(ox0, sw, W, wx0, unused, lu);
  cr_src(ox1, sw, W, unused, wx1, lu);
  const int wrows = wy1 - wy0 + 1, wcols = wx1 - wx0 + 1;
  const int wtotal = min(wrows * wcols, win_cap);   // (the entry point sized win_cap to hold every tile's window)
  __syncthreads();
  const float ub0 = u1_b[0], ub1 = u1_b[1];
  const float* lon = low + (long long)n * h * w * 2;
  const float2* tnn = reinterpret_cast<const float2*>(tn2) + (long long)n * H * W;
  for (int i = t; i < wtotal; i += 256) {
    const int Y = wy0 + i / wcols, X = wx0 + i % wcols;
    const int dy = Y & 1, dx = X & 1;
    const float* lo = lon + ((long long)(Y >> 1) * w + (X >> 1)) * 2;
    const float l0 = lo[0], l1 = lo[1];
    float b0 = ub0, b1 = ub1;
    for (int co = 0; co < 32; ++co) {
      // ConvTranspose2d weight [ci][co][dy][dx]
      float hsum = l0 * s_ut[((0 * 32 + co) * 2 + dy) * 2 + dx] + l1 * s_ut[((1 * 32 + co) * 2 + dy) * 2 + dx];
      hsum = apply_act(hsum * s_us[co] + s_ush[co], ut_act, ut_beta);
      b0 += s_u1[co] * hsum;
      b1 += s_u1[32 + co] * hsum;
    }
    const float2 tq = tnn[(long long)Y * W + X];
    s_win[i] = make_float4(b0, b1, tq.x, tq.y);
  }
  __syncthreads();
  const int oy = oy0 + (t >> tw_log2), ox = ox0 + (t & (TW - 1));
  if (oy >= mh || ox >= mw) return;
  int y0, y1, x0, x1;
  float ly, lx;
  cr_src(oy, sh, H, y0, y1, ly);
  cr_src(ox, sw, W, x0, x1, lx);
  const int last = wtotal - 1;
  const float4 p00 = s_win[min((y0 - wy0) * wcols + (x0 - wx0), last)];
  const float4 p01 = s_win[min((y0 - wy0) * wcols + (x1 - wx0), last)];
  const float4 p10 = s_win[min((y1 - wy0) * wcols + (x0 - wx0), last)];
  const float4 p11 = s_win[min((y1 - wy0) * wcols + (x1 - wx0), last)];
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float b0 = hy * (hx * p00.x + lx * p01.x) + ly * (hx * p10.x + lx * p11.x);
  const float b1 = hy * (hx * p00.y + lx * p01.y) + ly * (hx * p10.y + lx * p11.y);
  const float t0 = hy * (hx * p00.z + lx * p01.z) + ly * (hx * p10.z + lx * p11.z);
  const float t1 = hy * (hx * p00.w + lx * p01.w) + ly * (hx * p10.w + lx * p11.w);
  const float mx = fmaxf(b0, b1);
  const float e0 = __expf(b0 - mx), e1 = __expf(b1 - mx);
  const float pfg = e1 / (e0 + e1);
  const long long plane = (long long)mh * mw;
  const long long pp = (long long)oy * mw + ox;
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

// Rows (or columns) of the source window of `tile` consecutive outputs at ratio in / out: the first taps of the first
// and last output are at most floor((tile - 1) * scale) + 1 apart, plus the last one's second tap; one more for the
// rounding of the float coordinate.  Never more than the source has.
static int cr_window(int tile, int in, int out) {
  const double scale = (double)in / (double)out;
  const long long n = (long long)((tile - 1) * scale) + 4;
  return (int)(n < in ? n : in);
}

}  // namespace hiseg

using namespace hiseg;

extern "C" int hiseg_hier_combine_resize(const float* low, int N, int h, int w, const float* tn2, const float* ut_w,
                                         const float* ut_scale, const float* ut_shift, int ut_act, float ut_beta,
                                         int ut_per_sample, const float* u1_w, const float* u1_b, int mh, int mw,
                                         float* logits, float* bgfg, float* tn, hiseg_stream_t stream) {
  HISEG_REQUIRE(low && tn2 && ut_w && ut_scale && ut_shift && u1_w && u1_b && logits, HISEG_ERR_BAD_ARG,
                "hier_combine_resize: null pointer");
  HISEG_REQUIRE(N >= 0 && h > 0 && w > 0 && mh > 0 && mw > 0 && h <= (1 << 14) && w <= (1 << 14) && mh <= (1 << 15) &&
                    mw <= (1 << 15) && ((uintptr_t)tn2 & 7) == 0,
                HISEG_ERR_BAD_SHAPE, "hier_combine_resize: bad shape (ROI %d x %d, mask %d x %d)", h, w, mh, mw);
  HISEG_REQUIRE(ut_act >= HISEG_ACT_NONE && ut_act <= HISEG_ACT_SWISH, HISEG_ERR_BAD_ARG,
                "hier_combine_resize: unknown activation %d", ut_act);
  if (N == 0) return HISEG_OK;
  const int tw_log2 = mw > 32 ? 6 : (mw > 16 ? 5 : 4);
  const int TW = 1 << tw_log2, TH = 256 >> tw_log2;
  const int win_cap = cr_window(TH, 2 * h, mh) * cr_window(TW, 2 * w, mw);
  HISEG_REQUIRE(win_cap <= kCrWindowMax, HISEG_ERR_BAD_SHAPE,
                "hier_combine_resize: mask %d x %d is too small a part of the %d x %d grid (source window of %d "
                "pixels per tile, at most %d)", mh, mw, 2 * h, 2 * w, win_cap, kCrWindowMax);
  const int tiles_x = (mw + TW - 1) / TW, tiles_y = (mh + TH - 1) / TH;
  const long long blocks = (long long)N * tiles_x * tiles_y;
  HISEG_REQUIRE(blocks < (1ll << 31), HISEG_ERR_BAD_SHAPE, "hier_combine_resize: too many tiles");
  hipLaunchKernelGGL(hier_combine_resize_kernel, dim3((unsigned)blocks), dim3(256), (size_t)win_cap * sizeof(float4),
                     (hipStream_t)stream, low, h, w, tn2, ut_w, ut_scale, ut_shift, ut_act, ut_beta,
                     ut_per_sample ? 32 : 0, u1_w, u1_b, mh, mw, tw_log2, tiles_x, tiles_y, win_cap, logits, bgfg, tn);
  return hiseg_check_launch("hier_combine_resize");
}
