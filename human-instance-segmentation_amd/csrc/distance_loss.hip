// Boundary distance transform, boundary weight map and DistanceAwareSegmentationLoss on gfx950 (see
// include/hiseg_distance.h).
//
// Distance transform (dist_kernel): one workgroup owns an output rectangle of one sample -- the whole mask in the
// LDS-resident form, a 64 x 64 tile in the halo-tiled form -- and holds in LDS the mask of the rectangle grown by the
// search radius (uint8, plus one border row / column up and left for the edge rule) and its row distances (uint16).
//   load   : mask region -> LDS; the resident form finds the sample's class set on the way, the tiled form reads it
//            from dist_classes_kernel's pre-pass (the site rule is per sample, not per tile)
//   sites  : g = 0 at a site, infinite elsewhere
//   rows   : one thread per region row, a forward and a backward running minimum: g = distance to the nearest site
//            of the row (row stride padded to an odd number of LDS words, so the threads of a wave hit distinct banks)
//   columns: per output pixel min over dy of g(y + dy)^2 + dy^2, outward from dy = 0 and stopping once dy^2 reaches
//            the best value so far; row distances above the radius are ignored (in a tile they may be wrong)
//   weights: the epilogue of the same kernel, from the integer d2 and the caller's double table
// Loss: per (sample, split) block partial sums in double -> one finalize block (per-sample dice, global means, the
// backward's coefficients) -> a per-pixel backward.  Shuffle + LDS reductions in a fixed order, no atomics.
//
// The helpers of train_loss.hip (softmax3, the dice statistics of loss_main_kernel) are local to that file and tied
// to its partial layout; the few lines needed here are restated so that file stays as it is.
#include "common.h"
#include "hiseg_distance.h"

// The weight is f32(1 + (bw - 1) * t) with both operations rounded in double, as numpy evaluates it; a fused
// multiply-add changes the last bit (the same happened to RoIAlign).
#pragma clang fp contract(off)

namespace hiseg {
namespace dist {   // (kernels keep external linkage, as everywhere in the library; the names are this file's)

constexpr int kT = 256;
constexpr int kLds = 160 * 1024;   // bytes of LDS a workgroup may use on gfx950
constexpr int kTile = 64;          // output tile edge of the halo-tiled form
constexpr int kInf = 0xFFFF;       // "no site in this row" (uint16)
constexpr int kMaxDim = 16384;     // g^2 + dy^2 stays below 2^31
constexpr int kSplit = 8;          // blocks per sample in the loss forward
constexpr int kNS = 10;            // sums per partial
enum { S_CEW = 0, S_W, S_C0, S_C1, S_C2, S_FOC, S_INT, S_PS, S_NB, S_NBC };

__host__ __device__ inline int g_stride(int rw) {   // uint16 elements; an odd number of 4-byte words
  int s = (rw + 1) & ~1;
  if ((s & 3) == 0) s += 2;
  return s;
}
__host__ __device__ inline long long mask_bytes(int rh, int rw) { return (((long long)(rh + 1) * (rw + 1)) + 15) & ~15LL; }
// LDS of a region: a 16-byte header (the class flags), the mask, the row distances.  All of it is dynamic: the kernel
// must hold no static LDS (__syncthreads_or brings 256 bytes of it), or raising the dynamic limit to 160 KB is refused.
constexpr int kHdr = 16;
__host__ __device__ inline long long region_lds(int rh, int rw) {
  return kHdr + mask_bytes(rh, rw) + 2LL * rh * g_stride(rw);
}

struct DistArgs {
  const long long* tg;
  int N, H, W, R, d2cap, tiles_y, tiles_x;   // tiles_x == 0: the resident form
  const int* flags;                          // tiled form: class bits per sample
  int* d2;
  float* wout;                               // optional weight map
  const double* table;
  int width2;
  double bw, isw;
  const float* dev_w;
  const float* inst;
  const unsigned char* present;
};

__global__ void __launch_bounds__(kT) dist_classes_kernel(const long long* __restrict__ tg, long long HW,
                                                          int* __restrict__ flags) {
  const long long* t = tg + (long long)blockIdx.x * HW;
  int bits = 0;
  for (long long i = threadIdx.x; i < HW; i += kT) bits |= 1 << ((int)t[i] & 3);
  const int c0 = __syncthreads_or(bits & 1), c1 = __syncthreads_or(bits & 2), c2 = __syncthreads_or(bits & 4);
  if (threadIdx.x == 0) flags[blockIdx.x] = (c0 ? 1 : 0) | (c1 ? 2 : 0) | (c2 ? 4 : 0);
}

__global__ void __launch_bounds__(kT) dist_kernel(DistArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dist_lds[];
  const int tid = threadIdx.x, H = a.H, W = a.W, R = a.R;
  int n, oy0 = 0, ox0 = 0, oh = H, ow = W;
  if (a.tiles_x == 0) {
    n = blockIdx.x;
  } else {
    const int per = a.tiles_y * a.tiles_x;
    n = blockIdx.x / per;
    const int t = blockIdx.x - n * per, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    oy0 = ty * kTile; ox0 = tx * kTile;
    oh = min(kTile, H - oy0); ow = min(kTile, W - ox0);
  }
  // the region: the output rectangle grown by the radius, clipped to the image
  const int ry0 = max(oy0 - R, 0), rx0 = max(ox0 - R, 0);
  const int ry1 = min(oy0 + oh + R, H), rx1 = min(ox0 + ow + R, W);
  const int rh = ry1 - ry0, rw = rx1 - rx0, mw = rw + 1, gs = g_stride(rw);
  int* fl = reinterpret_cast<int*>(dist_lds);
  unsigned char* m = dist_lds + kHdr;
  unsigned short* g = reinterpret_cast<unsigned short*>(dist_lds + kHdr + mask_bytes(rh, rw));
  if (tid < 3) fl[tid] = 0;
  __syncthreads();
  const long long HW = (long long)H * W;
  const long long* tn = a.tg + (long long)n * HW;

  // mask of the region with one border row above and one border column to the left: the neighbour's value, or a
  // replicate at the image border (no edge there: np.diff(..., prepend=first row / column))
  int bits = 0;
  for (int i = tid; i < (rh + 1) * mw; i += kT) {
    const int ly = i / mw, lx = i - ly * mw;
    const int y = max(ry0 + ly - 1, 0), x = max(rx0 + lx - 1, 0);
    const int v = (int)tn[(long long)y * W + x] & 3;
    m[i] = (unsigned char)v;
    bits |= 1 << v;
  }
  // class set of the sample: every thread that saw a class stores the same 1 (no atomic, no order to depend on)
  if (bits & 1) fl[0] = 1;
  if (bits & 2) fl[1] = 1;
  if (bits & 4) fl[2] = 1;
  __syncthreads();
  const int cls = a.flags ? a.flags[n] : (fl[0] | (fl[1] << 1) | (fl[2] << 2));
  const bool three = cls == 7;
  const bool has_site = three || (cls & 2);   // three values always hold an edge; otherwise the sites are the 1s

  if (has_site) {
    for (int i = tid; i < rh * rw; i += kT) {
      const int ly = i / rw, lx = i - ly * rw;
      const int c = m[(ly + 1) * mw + lx + 1];
      const bool site = three ? (c != m[ly * mw + lx + 1] || c != m[(ly + 1) * mw + lx]) : c == 1;
      g[ly * gs + lx] = site ? 0 : kInf;
    }
    __syncthreads();
    for (int r = tid; r < rh; r += kT) {
      unsigned short* gr = g + r * gs;
      int run = kInf;
      for (int x = 0; x < rw; ++x) {
        run = gr[x] == 0 ? 0 : min(run + 1, kInf);
        gr[x] = (unsigned short)run;
      }
      run = kInf;
      for (int x = rw - 1; x >= 0; --x) {
        run = min((int)gr[x], min(run + 1, kInf));
        gr[x] = (unsigned short)run;
      }
    }
    __syncthreads();
  }

  double bw = a.bw;
  float isw = (float)a.isw;
  if (a.dev_w) { bw = (double)a.dev_w[0]; isw = a.dev_w[1]; }
  const bool inst = a.inst != nullptr && a.present[n] != 0;
  for (int i = tid; i < oh * ow; i += kT) {
    const int oy = i / ow, y = oy0 + oy, x = ox0 + (i - oy * ow);
    int best;
    if (!has_site) {
      best = (y + 1) * (y + 1) + x * x;   // the virtual site at (-1, 0)
    } else {
      best = 0x7FFFFFFF;
      const int ly = y - ry0, lx = x - rx0;
      for (int k = 0; k <= R; ++k) {
        if (k * k >= best) break;
        const bool up = ly - k >= 0, dn = ly + k < rh;
        if (!up && !dn) break;
        if (up) {
          const int gv = g[(ly - k) * gs + lx];
          if (gv <= R) best = min(best, gv * gv + k * k);
        }
        if (dn && k) {
          const int gv = g[(ly + k) * gs + lx];
          if (gv <= R) best = min(best, gv * gv + k * k);
        }
      }
    }
    const int v = min(best, a.d2cap);
    const long long o = (long long)n * HW + (long long)y * W + x;
    a.d2[o] = v;
    if (a.wout) {
      float w = 1.0f;
      if (v < a.width2) {
        const double s = 1.0 + (bw - 1.0) * a.table[v];
        w = (float)s;
      }
      if (inst && a.inst[o] < 50.0f) w = w * isw;
      a.wout[o] = w;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ loss
// workspace (floats): [0, 8) coefficients {ce coefficient, dice weight / N}; then as doubles from float 8 the
// partials [N * kSplit][kNS]; then float [N][2] per-sample dice coefficients; then (8-byte aligned) int flags [N]
struct LossWs {
  float* coef;
  double* part;
  float* dcoef;
  int* flags;
};
__host__ __device__ inline LossWs dl_ws(float* ws, int N) {
  LossWs w;
  w.coef = ws;
  w.part = reinterpret_cast<double*>(ws + 8);
  w.dcoef = ws + 8 + 2LL * N * kSplit * kNS;
  w.flags = reinterpret_cast<int*>(w.dcoef + 2LL * N);
  return w;
}

// sum of v over the block in a fixed order (wave shuffles, then the four waves in order); valid on thread 0
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sh /* [4 * K] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = v[k];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) sh[wave * K + k] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((sh[k] + sh[K + k]) + sh[2 * K + k]) + sh[3 * K + k];
  }
}

struct Pixel {
  float p[3], ce;
  int t;
};
__device__ __forceinline__ Pixel load_pixel(const float* __restrict__ pn, const long long* __restrict__ tn,
                                            long long r, long long HW, float (&x)[3]) {
  Pixel q;
  x[0] = pn[r]; x[1] = pn[HW + r]; x[2] = pn[2 * HW + r];
  const long long t = tn[r];
  q.t = t < 0 ? 0 : (t > 2 ? 2 : (int)t);
  const float mx = fmaxf(x[0], fmaxf(x[1], x[2]));
  const float e0 = expf(x[0] - mx), e1 = expf(x[1] - mx), e2 = expf(x[2] - mx);
  const float s = (e0 + e1) + e2;
  q.p[0] = e0 / s; q.p[1] = e1 / s; q.p[2] = e2 / s;
  q.ce = -((x[q.t] - mx) - logf(s));   // -log_softmax(x)[t]
  return q;
}

__global__ void __launch_bounds__(kT) dl_main_kernel(const float* __restrict__ pred, const long long* __restrict__ tg,
                                                     const float* __restrict__ wmap, int N, long long HW,
                                                     const float* __restrict__ cw, int use_focal, float gamma,
                                                     double* __restrict__ part) {
  const int n = blockIdx.x / kSplit, s = blockIdx.x - n * kSplit;
  const long long chunk = (HW + kSplit - 1) / kSplit;
  const long long r0 = s * chunk, r1 = min(r0 + chunk, HW);
  const float* pn = pred + (long long)n * 3 * HW;
  const long long* tn = tg + (long long)n * HW;
  const float* wn = wmap + (long long)n * HW;
  float alpha[3] = {1.f, 1.f, 1.f};
  if (cw) { alpha[0] = cw[0]; alpha[1] = cw[1]; alpha[2] = cw[2]; }
  double acc[kNS];
#pragma unroll
  for (int k = 0; k < kNS; ++k) acc[k] = 0.0;
  for (long long r = r0 + threadIdx.x; r < r1; r += kT) {
    float x[3];
    const Pixel q = load_pixel(pn, tn, r, HW, x);
    const float w = wn[r];
    acc[S_CEW] += (double)(q.ce * w);
    acc[S_W] += (double)w;
    acc[S_C0 + q.t] += 1.0;
    if (use_focal) {
      const float pt = expf(-q.ce);
      acc[S_FOC] += (double)(alpha[q.t] * (powf(1.0f - pt, gamma) * q.ce));
    }
    if (q.t == 1) acc[S_INT] += (double)q.p[1];
    acc[S_PS] += (double)q.p[1];
    if (w > 1.5f) {
      int am = 0;
      if (x[1] > x[am]) am = 1;
      if (x[2] > x[am]) am = 2;
      acc[S_NB] += 1.0;
      if (am == q.t) acc[S_NBC] += 1.0;
    }
  }
  __shared__ double sh[4 * kNS];
  block_sum<kNS>(acc, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kNS; ++k) part[(long long)blockIdx.x * kNS + k] = acc[k];
  }
}

__global__ void __launch_bounds__(kT) dl_finalize_kernel(LossWs w, int N, long long HW, const float* __restrict__ cw,
                                                         int use_focal, float ce_weight, float dice_weight,
                                                         float* __restrict__ out) {
  // 0 cew, 1 w, 2-4 class counts, 5 focal, 6 boundary pixels, 7 correct boundary pixels, 8 dice
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  for (int n = threadIdx.x; n < N; n += kT) {
    double s[kNS];
#pragma unroll
    for (int k = 0; k < kNS; ++k) s[k] = 0.0;
    for (int j = 0; j < kSplit; ++j)
#pragma unroll
      for (int k = 0; k < kNS; ++k) s[k] += w.part[((long long)n * kSplit + j) * kNS + k];
    const double num = 2.0 * s[S_INT] + 1e-6, den = s[S_PS] + s[S_C1] + 1e-6;
    w.dcoef[2 * n] = (float)(2.0 / den);
    w.dcoef[2 * n + 1] = (float)(num / (den * den));
    acc[0] += s[S_CEW]; acc[1] += s[S_W]; acc[2] += s[S_C0]; acc[3] += s[S_C1]; acc[4] += s[S_C2];
    acc[5] += s[S_FOC]; acc[6] += s[S_NB]; acc[7] += s[S_NBC];
    acc[8] += 1.0 - num / den;
  }
  __shared__ double sh[4 * 9];
  block_sum<9>(acc, sh);
  if (threadIdx.x == 0) {
    const double P = (double)N * (double)HW;
    const double mean_w = acc[1] / P;
    double K = 1.0;   // mean(class_weights[target]): the reference multiplies the scalar by the map and averages
    if (cw) K = ((double)cw[0] * acc[2] + (double)cw[1] * acc[3] + (double)cw[2] * acc[4]) / P;
    double wce, coef;
    if (use_focal) {
      wce = (acc[5] / P) * mean_w * K;
      coef = (double)ce_weight * K * mean_w / P;
    } else {
      wce = (acc[0] / P) * K;
      coef = (double)ce_weight * K / P;
    }
    const double dice = acc[8] / (double)N;
    out[0] = (float)((double)ce_weight * wce + (double)dice_weight * dice);
    out[1] = (float)wce;
    out[2] = (float)dice;
    out[3] = acc[6] > 0.0 ? (float)(acc[7] / acc[6]) : 0.f;
    out[4] = (float)mean_w;
    out[5] = out[6] = out[7] = 0.f;
    w.coef[0] = (float)coef;
    w.coef[1] = (float)((double)dice_weight / (double)N);
  }
}

__global__ void __launch_bounds__(kT) dl_bwd_kernel(const float* __restrict__ pred, const long long* __restrict__ tg,
                                                    const float* __restrict__ wmap, int N, long long HW,
                                                    const float* __restrict__ cw, int use_focal, float gamma,
                                                    LossWs w, const float* __restrict__ gscale,
                                                    float* __restrict__ dpred) {
  const long long P = (long long)N * HW;
  const float gs = gscale[0];
  const float kce = gs * w.coef[0], kdice = gs * w.coef[1];
  float alpha[3] = {1.f, 1.f, 1.f};
  if (cw) { alpha[0] = cw[0]; alpha[1] = cw[1]; alpha[2] = cw[2]; }
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    float x[3];
    const Pixel q = load_pixel(pred + n * 3 * HW, tg + n * HW, r, HW, x);
    // d (ce term) / d ce at this pixel
    float dce;
    if (use_focal) {
      const float pt = expf(-q.ce), b = 1.0f - pt;
      // d/dce [(1 - e^-ce)^gamma ce] = gamma (1 - pt)^(gamma - 1) pt ce + (1 - pt)^gamma
      dce = kce * alpha[q.t] * (gamma * powf(b, gamma - 1.0f) * pt * q.ce + powf(b, gamma));
    } else {
      dce = kce * wmap[i];
    }
    // d dice / d p1 = -(1/N) (2 t1 / D - (2 I + s) / D^2)
    const float dp1 = -kdice * ((q.t == 1 ? w.dcoef[2 * n] : 0.f) - w.dcoef[2 * n + 1]);
    const float dq = dp1 * q.p[1];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dpred[(n * 3 + c) * HW + r] = dce * (q.p[c] - (c == q.t ? 1.f : 0.f)) + dq * ((c == 1 ? 1.f : 0.f) - q.p[c]);
  }
}

static int check_dims(const char* what, int N, int H, int W) {
  HISEG_REQUIRE(N >= 1 && H >= 1 && W >= 1, HISEG_ERR_BAD_SHAPE, "%s: N %d H %d W %d", what, N, H, W);
  HISEG_REQUIRE(H <= kMaxDim && W <= kMaxDim, HISEG_ERR_BAD_SHAPE, "%s: H %d W %d above %d", what, H, W, kMaxDim);
  HISEG_REQUIRE((long long)N * kSplit <= 0x7FFFFFFF / 64, HISEG_ERR_BAD_SHAPE, "%s: N %d too large", what, N);
  return HISEG_OK;
}

static bool resident(int H, int W) { return region_lds(H, W) <= kLds; }

static int launch_dist(const char* what, DistArgs a, int force_tiled, float* ws, hiseg_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipFuncSetAttribute((const void*)dist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  HISEG_REQUIRE(e == hipSuccess, HISEG_ERR_LAUNCH, "%s: LDS limit: %s", what, hipGetErrorString(e));
  if (!force_tiled && resident(a.H, a.W)) {
    a.tiles_x = a.tiles_y = 0;
    a.flags = nullptr;
    hipLaunchKernelGGL(dist_kernel, dim3(a.N), dim3(kT), (size_t)region_lds(a.H, a.W), s, a);
    return hiseg_check_launch(what);
  }
  HISEG_REQUIRE(a.R <= HISEG_DISTANCE_MAX_HALO, HISEG_ERR_BAD_SHAPE,
                "%s: a %d x %d mask is not LDS-resident and the halo-tiled form takes a radius <= %d (got %d)", what,
                a.H, a.W, HISEG_DISTANCE_MAX_HALO, a.R);
  HISEG_REQUIRE(ws, HISEG_ERR_BAD_ARG, "%s: the halo-tiled form needs the workspace", what);
  a.tiles_y = (a.H + kTile - 1) / kTile;
  a.tiles_x = (a.W + kTile - 1) / kTile;
  const long long blocks = (long long)a.N * a.tiles_y * a.tiles_x;
  HISEG_REQUIRE(blocks <= 0x7FFFFFFF, HISEG_ERR_BAD_SHAPE, "%s: %lld tiles", what, blocks);
  int* flags = dl_ws(ws, a.N).flags;
  hipLaunchKernelGGL(dist_classes_kernel, dim3(a.N), dim3(kT), 0, s, a.tg, (long long)a.H * a.W, flags);
  a.flags = flags;
  const int edge = kTile + 2 * a.R;   // the largest region of a tile (region_lds grows with both edges)
  hipLaunchKernelGGL(dist_kernel, dim3((unsigned)blocks), dim3(kT), (size_t)region_lds(edge, edge), s, a);
  return hiseg_check_launch(what);
}

}  // namespace dist
}  // namespace hiseg

using namespace hiseg;
using namespace hiseg::dist;

extern "C" int hiseg_distance_resident(int H, int W) {
  return H >= 1 && W >= 1 && H <= kMaxDim && W <= kMaxDim && resident(H, W) ? 1 : 0;
}

extern "C" long long hiseg_distance_ws(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  return 8 + 2LL * N * kSplit * kNS + 2LL * N + N + 8;
}

extern "C" int hiseg_distance_transform(const long long* target, int N, int H, int W, int radius, int d2cap,
                                        int force_tiled, int* d2, float* ws, hiseg_stream_t stream) {
  if (int st = check_dims("distance_transform", N, H, W)) return st;
  HISEG_REQUIRE(target && d2, HISEG_ERR_BAD_ARG, "distance_transform: null pointer");
  HISEG_REQUIRE(radius >= 0 && d2cap >= 1, HISEG_ERR_BAD_ARG, "distance_transform: radius %d, d2cap %d", radius, d2cap);
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, HISEG_ERR_BAD_SHAPE, "distance_transform: ws alignment");
  DistArgs a = {};
  a.tg = target; a.N = N; a.H = H; a.W = W;
  a.R = radius < (H > W ? H : W) ? radius : (H > W ? H : W);
  a.d2cap = d2cap;
  a.d2 = d2;
  return launch_dist("distance_transform", a, force_tiled, ws, stream);
}

extern "C" int hiseg_distance_weight_map(const long long* target, int N, int H, int W, int width, const double* table,
                                         double boundary_weight, double instance_sep_weight, const float* dev_weights,
                                         const float* inst_dist, const unsigned char* inst_present, int force_tiled,
                                         int* d2, float* weights, float* ws, hiseg_stream_t stream) {
  if (int st = check_dims("distance_weight_map", N, H, W)) return st;
  HISEG_REQUIRE(target && table && d2 && weights, HISEG_ERR_BAD_ARG, "distance_weight_map: null pointer");
  HISEG_REQUIRE(width >= 1 && width <= kMaxDim, HISEG_ERR_BAD_ARG, "distance_weight_map: boundary width %d", width);
  HISEG_REQUIRE((inst_dist == nullptr) == (inst_present == nullptr), HISEG_ERR_BAD_ARG,
                "distance_weight_map: inst_dist and inst_present come together");
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, HISEG_ERR_BAD_SHAPE, "distance_weight_map: ws alignment");
  DistArgs a = {};
  a.tg = target; a.N = N; a.H = H; a.W = W;
  const int mx = H > W ? H : W;
  a.R = width - 1 < mx ? width - 1 : mx;
  a.d2cap = a.width2 = width * width;
  a.d2 = d2; a.wout = weights; a.table = table;
  a.bw = boundary_weight; a.isw = instance_sep_weight; a.dev_w = dev_weights;
  a.inst = inst_dist; a.present = inst_present;
  return launch_dist("distance_weight_map", a, force_tiled, ws, stream);
}

extern "C" int hiseg_distance_loss_fwd(const float* pred, const long long* target, const float* weights, int N, int H,
                                       int W, const float* class_weights, int use_focal, float focal_gamma,
                                       float ce_weight, float dice_weight, float* ws, float* out,
                                       hiseg_stream_t stream) {
  if (int st = check_dims("distance_loss_fwd", N, H, W)) return st;
  HISEG_REQUIRE(pred && target && weights && ws && out, HISEG_ERR_BAD_ARG, "distance_loss_fwd: null pointer");
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, HISEG_ERR_BAD_SHAPE, "distance_loss_fwd: ws alignment");
  hipStream_t s = (hipStream_t)stream;
  const LossWs w = dl_ws(ws, N);
  const long long HW = (long long)H * W;
  hipLaunchKernelGGL(dl_main_kernel, dim3(N * kSplit), dim3(kT), 0, s, pred, target, weights, N, HW, class_weights,
                     use_focal, focal_gamma, w.part);
  hipLaunchKernelGGL(dl_finalize_kernel, dim3(1), dim3(kT), 0, s, w, N, HW, class_weights, use_focal, ce_weight,
                     dice_weight, out);
  return hiseg_check_launch("distance_loss_fwd");
}

extern "C" int hiseg_distance_loss_bwd(const float* pred, const long long* target, const float* weights, int N, int H,
                                       int W, const float* class_weights, int use_focal, float focal_gamma,
                                       const float* ws, const float* gscale, float* dpred, hiseg_stream_t stream) {
  if (int st = check_dims("distance_loss_bwd", N, H, W)) return st;
  HISEG_REQUIRE(pred && target && weights && ws && gscale && dpred, HISEG_ERR_BAD_ARG,
                "distance_loss_bwd: null pointer");
  const LossWs w = dl_ws(const_cast<float*>(ws), N);
  const long long HW = (long long)H * W, P = (long long)N * HW;
  const long long blocks = (P + kT - 1) / kT;
  hipLaunchKernelGGL(dl_bwd_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kT), 0, (hipStream_t)stream,
                     pred, target, weights, N, HW, class_weights, use_focal, focal_gamma, w, gscale, dpred);
  return hiseg_check_launch("distance_loss_bwd");
}
