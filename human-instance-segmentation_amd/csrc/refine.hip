// Boundary refinement stage and active-contour loss (include/hiseg_refine.h).
//
//   edge_raw      : per pixel softmax of the pixel and its +1 neighbours, the replicate-padded differences, raw e,
//                   block partials of the min / max (+ optional probs and the channel-last copy of x)
//   edge_minmax   : one block reduces the partials to the device pair [mn, mx]
//   blend_fwd     : out = x + (blend * R) * E, the flat branch (mx - mn < 1e-6) taken on the device
//   blend_bwd     : dR, d loss / d E, block partials (double) of dblend, sum dE, sum dE (e - mn), tie counts
//   blend_sums    : one block sums the partials in a fixed order
//   edge_bwd_a    : per pixel the gradient of its own y / x difference (replicated rows / columns gathered in)
//   edge_bwd_b    : per pixel gather of the difference gradients, softmax backward, + g + conv-path gradient
//   ac_prob / ac_sum / ac_final / ac_bwd : the active-contour term on the class-1 probability
//
// All arithmetic is f32 in the reference's operation order (double only inside the fixed-order reductions); the
// backward has no special case at zero (the sqrt's 0/0 is the reference's NaN).
#include "common.h"
#include "gfx950_prims.h"
#include "hiseg_refine.h"

#include <math.h>

namespace {

constexpr int kT = 256;        // threads per block
constexpr int kMaxBlk = 1024;  // blocks of a grid-stride launch == rows of a partials table

inline int grid_for(long long P) {
  const long long b = (P + kT - 1) / kT;
  return (int)(b < kMaxBlk ? b : kMaxBlk);
}

// softmax over the 3 channel planes at pixel offset `at` of sample base `x` (planes HW apart)
__device__ __forceinline__ void softmax3(const float* x, long long at, long long HW, float* p) {
  const float a = x[at], b = x[at + HW], c = x[at + 2 * HW];
  const float m = fmaxf(a, fmaxf(b, c));
  const float ea = expf(a - m), eb = expf(b - m), ec = expf(c - m);
  const float s = ea + eb + ec;
  p[0] = ea / s;
  p[1] = eb / s;
  p[2] = ec / s;
}

__device__ __forceinline__ float sgnf(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// ------------------------------------------------------------------------------------------------ forward
__global__ void __launch_bounds__(kT) edge_raw_kernel(const float* __restrict__ x, int N, int H, int W,
                                                      float* __restrict__ e, float* __restrict__ probs,
                                                      void* __restrict__ xcl, int cl_bf16, int cl_cs,
                                                      float* __restrict__ part) {
  const long long HW = (long long)H * W, P = (long long)N * HW;
  float mn = INFINITY, mx = -INFINITY;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    const int h = (int)(r / W), w = (int)(r - (long long)h * W);
    const int hh = h < H - 2 ? h : H - 2, ww = w < W - 2 ? w : W - 2;
    const float* xs = x + n * 3 * HW;
    float ylo[3], yhi[3], xlo[3], xhi[3];
    softmax3(xs, (long long)hh * W + w, HW, ylo);
    softmax3(xs, (long long)(hh + 1) * W + w, HW, yhi);
    softmax3(xs, (long long)h * W + ww, HW, xlo);
    softmax3(xs, (long long)h * W + ww + 1, HW, xhi);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float dy = fabsf(yhi[c] - ylo[c]), dx = fabsf(xhi[c] - xlo[c]);
      s += sqrtf(dy * dy + dx * dx);
    }
    const float ev = s / 3.0f;
    e[i] = ev;
    mn = fminf(mn, ev);
    mx = fmaxf(mx, ev);
    if (probs) {
      const float* self = h == hh ? ylo : yhi;
#pragma unroll
      for (int c = 0; c < 3; ++c) probs[(n * 3 + c) * HW + r] = self[c];
    }
    if (xcl) {   // one packed store per pixel at the usual strides (8 bf16 / 4 f32: 16 B), element-wise otherwise
      const float v0 = xs[r], v1 = xs[HW + r], v2 = xs[2 * HW + r];
      if (cl_bf16 && cl_cs == 8) {
        reinterpret_cast<uint4*>(xcl)[i] = make_uint4(hiseg::f2bf2(v0, v1), hiseg::f2bf2(v2, 0.f), 0u, 0u);
      } else if (!cl_bf16 && cl_cs == 4) {
        reinterpret_cast<float4*>(xcl)[i] = make_float4(v0, v1, v2, 0.f);
      } else {
        for (int c = 0; c < cl_cs; ++c) {
          const float v = c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : 0.f;
          if (cl_bf16) reinterpret_cast<uint16_t*>(xcl)[i * cl_cs + c] = hiseg::f2bf(v);
          else reinterpret_cast<float*>(xcl)[i * cl_cs + c] = v;
        }
      }
    }
  }
  __shared__ float smn[kT], smx[kT];
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + s]);
      smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = smn[0];
    part[2 * blockIdx.x + 1] = smx[0];
  }
}

__global__ void __launch_bounds__(kT) edge_minmax_kernel(const float* __restrict__ part, int nblk,
                                                         float* __restrict__ mnmx) {
  __shared__ float smn[kT], smx[kT];
  float mn = INFINITY, mx = -INFINITY;
  for (int b = threadIdx.x; b < nblk; b += kT) {
    mn = fminf(mn, part[2 * b]);
    mx = fmaxf(mx, part[2 * b + 1]);
  }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + s]);
      smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mnmx[0] = smn[0];
    mnmx[1] = smx[0];
  }
}

__global__ void __launch_bounds__(kT) blend_fwd_kernel(const float* __restrict__ x, const float* __restrict__ R,
                                                       int r_cs, const float* __restrict__ e,
                                                       const float* __restrict__ mnmx,
                                                       const float* __restrict__ blend, int N, int H, int W,
                                                       float* __restrict__ out, float* __restrict__ E_out) {
  const long long HW = (long long)H * W, P = (long long)N * HW;
  const float mn = mnmx[0], mx = mnmx[1], b = blend[0];
  const bool flat = mx - mn < 1e-6f;
  const float D = mx - mn + 1e-6f;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    const float E = flat ? 0.f : (e[i] - mn) / D;
    if (E_out) E_out[i] = E;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long at = (n * 3 + c) * HW + r;
      out[at] = x[at] + (b * R[i * r_cs + c]) * E;
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
// workspace of the backward (floats): [0, 16 + 10 * kMaxBlk) doubles region (sums[8] then partials[kMaxBlk][5]),
// then dE [P], then A [P][6]
struct BwdWs {
  double* sums;   // S0, S1, count(min), count(max), dblend
  double* part;
  float* dE;
  float* A;
};
__host__ __device__ inline BwdWs bwd_ws(float* ws, long long P) {
  BwdWs w;
  w.sums = reinterpret_cast<double*>(ws);
  w.part = w.sums + 8;
  w.dE = ws + 16 + 10 * kMaxBlk;
  w.A = w.dE + P;
  return w;
}

template <int K>
__device__ __forceinline__ void block_sum_store(double (&v)[K], double* sh, double* dst) {
  // fixed-order tree over the block's threads; dst[k] = sum
  for (int k = 0; k < K; ++k) {
    sh[threadIdx.x] = v[k];
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) dst[k] = sh[0];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kT) blend_bwd_kernel(const float* __restrict__ g, const float* __restrict__ R,
                                                       int r_cs, const float* __restrict__ e,
                                                       const float* __restrict__ mnmx,
                                                       const float* __restrict__ blend, int N, int H, int W,
                                                       float* __restrict__ dR, int dr_cs, float* __restrict__ dE,
                                                       double* __restrict__ part) {
  const long long HW = (long long)H * W, P = (long long)N * HW;
  const float mn = mnmx[0], mx = mnmx[1], b = blend[0];
  const bool flat = mx - mn < 1e-6f;
  const float D = mx - mn + 1e-6f;
  double acc[5] = {0, 0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    const float ev = e[i];
    const float E = flat ? 0.f : (ev - mn) / D;
    float de = 0.f, db = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gv = g[(n * 3 + c) * HW + r], rv = R[i * r_cs + c];
      const float t = gv * E;   // d (blend * R)
      dR[i * dr_cs + c] = t * b;
      db += t * rv;
      de += gv * (b * rv);
    }
    for (int c = 3; c < dr_cs; ++c) dR[i * dr_cs + c] = 0.f;
    dE[i] = de;
    acc[0] += (double)de;
    acc[1] += (double)(de * (ev - mn));
    acc[2] += ev == mn ? 1.0 : 0.0;
    acc[3] += ev == mx ? 1.0 : 0.0;
    acc[4] += (double)db;
  }
  __shared__ double sh[kT];
  block_sum_store<5>(acc, sh, part + 5 * blockIdx.x);
}

__global__ void __launch_bounds__(kT) blend_sums_kernel(const double* __restrict__ part, int nblk,
                                                        double* __restrict__ sums, float* __restrict__ dblend) {
  double acc[5] = {0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblk; b += kT)
    for (int k = 0; k < 5; ++k) acc[k] += part[5 * b + k];
  __shared__ double sh[kT];
  block_sum_store<5>(acc, sh, sums);
  if (threadIdx.x == 0 && dblend) dblend[0] += (float)sums[4];
}

// Gradient that pixel (h, w) of sample n sends to its own y difference (cy, living at row min(h, H-2)) and x
// difference (cx, at column min(w, W-2)): mean backward (/3), sqrt backward (/ (2 m)), square backward (* 2 d), abs
// backward (* sgn) -- plain IEEE, m == 0 gives NaN.
__device__ __forceinline__ void pixel_contrib(const float* __restrict__ ps, const float* __restrict__ e,
                                              const float* __restrict__ dE, long long i, int h, int w, int H, int W,
                                              long long HW, bool flat, float mn, float mx, float D, float dmn,
                                              float dmx, float* cy, float* cx) {
  const int hh = h < H - 2 ? h : H - 2, ww = w < W - 2 ? w : W - 2;
  float de = 0.f;
  if (!flat) {
    de = dE[i] / D;
    const float ev = e[i];
    if (ev == mn) de += dmn;
    if (ev == mx) de += dmx;
  }
  const float dm = de / 3.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* pc = ps + c * HW;
    const float vy = pc[(long long)(hh + 1) * W + w] - pc[(long long)hh * W + w];
    const float vx = pc[(long long)h * W + ww + 1] - pc[(long long)h * W + ww];
    const float ay = fabsf(vy), ax = fabsf(vx);
    const float m = sqrtf(ay * ay + ax * ax);
    const float t = dm / (2.0f * m);
    cy[c] = (t * (2.0f * ay)) * sgnf(vy);
    cx[c] = (t * (2.0f * ax)) * sgnf(vx);
  }
}

__global__ void __launch_bounds__(kT) edge_bwd_a_kernel(const float* __restrict__ probs, const float* __restrict__ e,
                                                        const float* __restrict__ mnmx, int N, int H, int W,
                                                        const double* __restrict__ sums,
                                                        const float* __restrict__ dE, float* __restrict__ A) {
  const long long HW = (long long)H * W, P = (long long)N * HW;
  const float mn = mnmx[0], mx = mnmx[1];
  const bool flat = mx - mn < 1e-6f;
  const float D = mx - mn + 1e-6f;
  float dmn = 0.f, dmx = 0.f;
  if (!flat) {   // gradient of the min / max, shared evenly by the tied elements
    const double Dd = (double)D;
    dmn = (float)((-sums[0] / Dd + sums[1] / (Dd * Dd)) / sums[2]);
    dmx = (float)((-sums[1] / (Dd * Dd)) / sums[3]);
  }
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    const int h = (int)(r / W), w = (int)(r - (long long)h * W);
    const float* ps = probs + n * 3 * HW;
    float ay[3] = {0.f, 0.f, 0.f}, ax[3] = {0.f, 0.f, 0.f};
    if (!flat) {
      float cy[3], cx[3];
      pixel_contrib(ps, e, dE, i, h, w, H, W, HW, flat, mn, mx, D, dmn, dmx, cy, cx);
      if (h <= H - 2)
        for (int c = 0; c < 3; ++c) ay[c] = cy[c];
      if (w <= W - 2)
        for (int c = 0; c < 3; ++c) ax[c] = cx[c];
      if (h == H - 2) {   // the replicated last row
        float by[3], bx[3];
        pixel_contrib(ps, e, dE, i + W, h + 1, w, H, W, HW, flat, mn, mx, D, dmn, dmx, by, bx);
        for (int c = 0; c < 3; ++c) ay[c] += by[c];
      }
      if (w == W - 2) {   // the replicated last column
        float by[3], bx[3];
        pixel_contrib(ps, e, dE, i + 1, h, w + 1, H, W, HW, flat, mn, mx, D, dmn, dmx, by, bx);
        for (int c = 0; c < 3; ++c) ax[c] += bx[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      A[i * 6 + c] = ay[c];
      A[i * 6 + 3 + c] = ax[c];
    }
  }
}

__global__ void __launch_bounds__(kT) edge_bwd_b_kernel(const float* __restrict__ g, const void* __restrict__ gcl,
                                                        int cl_bf16, int cl_cs, const float* __restrict__ probs,
                                                        const float* __restrict__ mnmx, int N, int H, int W,
                                                        const float* __restrict__ A, float* __restrict__ dx) {
  const long long HW = (long long)H * W, P = (long long)N * HW;
  const bool flat = mnmx[1] - mnmx[0] < 1e-6f;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    const int h = (int)(r / W), w = (int)(r - (long long)h * W);
    float de[3] = {0.f, 0.f, 0.f};
    if (!flat) {
      float dp[3], p[3], dot = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = 0.f;
        if (h >= 1) v += A[(i - W) * 6 + c];
        if (h <= H - 2) v -= A[i * 6 + c];
        if (w >= 1) v += A[(i - 1) * 6 + 3 + c];
        if (w <= W - 2) v -= A[i * 6 + 3 + c];
        dp[c] = v;
        p[c] = probs[(n * 3 + c) * HW + r];
        dot += v * p[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) de[c] = (dp[c] - dot) * p[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = g[(n * 3 + c) * HW + r];
      if (gcl) {
        v += cl_bf16 ? hiseg::bf2f(reinterpret_cast<const uint16_t*>(gcl)[i * cl_cs + c])
                     : reinterpret_cast<const float*>(gcl)[i * cl_cs + c];
      }
      dx[(n * 3 + c) * HW + r] = v + de[c];
    }
  }
}

// ------------------------------------------------------------------------------------------------ active contour
// workspace (floats): [0, 2) the forward's out pair, [8, 8 + 8 * kMaxBlk) double partials [kMaxBlk][4], then q [P]
__host__ __device__ inline double* ac_part(float* ws) { return reinterpret_cast<double*>(ws + 8); }
__host__ __device__ inline float* ac_q(float* ws) { return ws + 8 + 8 * kMaxBlk; }

__global__ void __launch_bounds__(kT) ac_prob_kernel(const float* __restrict__ pred, int N, long long HW,
                                                     float* __restrict__ q) {
  const long long P = (long long)N * HW;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    float p[3];
    softmax3(pred + n * 3 * HW, r, HW, p);
    q[i] = p[1];
  }
}

__global__ void __launch_bounds__(kT) ac_sum_kernel(const float* __restrict__ q, int N, int H, int W,
                                                    double* __restrict__ part) {
  const long long HW = (long long)H * W, P = (long long)N * HW;
  double acc[4] = {0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long r = i % HW;
    const int h = (int)(r / W), w = (int)(r - (long long)h * W);
    if (h <= H - 2) {
      const float d0 = q[i + W] - q[i];
      acc[0] += (double)fminf(fabsf(d0), 10.0f);
      if (h <= H - 3) acc[2] += (double)fabsf((q[i + 2 * W] - q[i + W]) - d0);
    }
    if (w <= W - 2) {
      const float d0 = q[i + 1] - q[i];
      acc[1] += (double)fminf(fabsf(d0), 10.0f);
      if (w <= W - 3) acc[3] += (double)fabsf((q[i + 2] - q[i + 1]) - d0);
    }
  }
  __shared__ double sh[kT];
  block_sum_store<4>(acc, sh, part + 4 * blockIdx.x);
}

__global__ void __launch_bounds__(kT) ac_final_kernel(const double* __restrict__ part, int nblk, int N, int H, int W,
                                                      float* __restrict__ hdr, float* __restrict__ out) {
  double acc[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblk; b += kT)
    for (int k = 0; k < 4; ++k) acc[k] += part[4 * b + k];
  __shared__ double sh[kT];
  __shared__ double tot[4];
  block_sum_store<4>(acc, sh, tot);
  if (threadIdx.x == 0) {
    const double n0 = (double)N * (H - 1) * W, n1 = (double)N * H * (W - 1);
    const double n2 = (double)N * (H - 2) * W, n3 = (double)N * H * (W - 2);
    const float len = (float)(tot[0] / n0) + (float)(tot[1] / n1);
    const float curv = (H >= 3 ? (float)(tot[2] / n2) : 0.f) + (W >= 3 ? (float)(tot[3] / n3) : 0.f);
    const float loss = len + 0.01f * curv;
    out[0] = hdr[0] = fminf(loss, 10.0f);
    out[1] = hdr[1] = loss;
  }
}

__global__ void __launch_bounds__(kT) ac_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ q,
                                                    const float* __restrict__ out, const float* __restrict__ gscale,
                                                    int N, int H, int W, float* __restrict__ dpred) {
  const long long HW = (long long)H * W, P = (long long)N * HW;
  // clamp(max=10) passes the gradient where loss <= 10
  const float gs = out[1] <= 10.0f ? gscale[0] : 0.f;
  const float gy = gs / (float)((double)N * (H - 1) * W), gx = gs / (float)((double)N * H * (W - 1));
  const float cyw = H >= 3 ? (gs * 0.01f) / (float)((double)N * (H - 2) * W) : 0.f;
  const float cxw = W >= 3 ? (gs * 0.01f) / (float)((double)N * H * (W - 2)) : 0.f;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < P; i += (long long)gridDim.x * kT) {
    const long long n = i / HW, r = i - n * HW;
    const int h = (int)(r / W), w = (int)(r - (long long)h * W);
    float dq = 0.f;
    // boundary length: s(k) = sgn(q[k+1] - q[k]) where |.| <= 10; dq[h] = s(h-1) - s(h)
    auto sy = [&](int k) {
      const float d = q[i + (long long)(k - h + 1) * W] - q[i + (long long)(k - h) * W];
      return fabsf(d) <= 10.0f ? sgnf(d) : 0.f;
    };
    auto sx = [&](int k) {
      const float d = q[i + (k - w + 1)] - q[i + (k - w)];
      return fabsf(d) <= 10.0f ? sgnf(d) : 0.f;
    };
    if (h >= 1) dq += gy * sy(h - 1);
    if (h <= H - 2) dq -= gy * sy(h);
    if (w >= 1) dq += gx * sx(w - 1);
    if (w <= W - 2) dq -= gx * sx(w);
    // curvature: c(k) = sgn((q[k+2] - q[k+1]) - (q[k+1] - q[k])), k in [0, H-3]; dq[h] = c(h) - 2 c(h-1) + c(h-2)
    auto cy = [&](int k) {
      const long long o = i + (long long)(k - h) * W;
      return sgnf((q[o + 2 * W] - q[o + W]) - (q[o + W] - q[o]));
    };
    auto cx = [&](int k) {
      const long long o = i + (k - w);
      return sgnf((q[o + 2] - q[o + 1]) - (q[o + 1] - q[o]));
    };
    if (h <= H - 3) dq += cyw * cy(h);
    if (h >= 1 && h <= H - 2) dq -= 2.0f * cyw * cy(h - 1);
    if (h >= 2) dq += cyw * cy(h - 2);
    if (w <= W - 3) dq += cxw * cx(w);
    if (w >= 1 && w <= W - 2) dq -= 2.0f * cxw * cx(w - 1);
    if (w >= 2) dq += cxw * cx(w - 2);
    float p[3];
    softmax3(pred + n * 3 * HW, r, HW, p);
    const float dot = dq * p[1];
#pragma unroll
    for (int c = 0; c < 3; ++c) dpred[(n * 3 + c) * HW + r] = ((c == 1 ? dq : 0.f) - dot) * p[c];
  }
}

// ------------------------------------------------------------------------------------------------ fused inference
// One workgroup (4 waves) per 16 x 16 tile of one sample.  LDS: the f32 logit tile with a halo of 2 (20 x 20 x 3,
// zero outside the image: conv1's padding), conv1's weights, and conv1's output at a halo of 1 as bf16
// [18 x 18][32] (zero outside the image: conv2's padding).  conv1 (K = 27) runs on the VALU, one position per
// thread and all 32 channels; conv2 is an implicit GEMM on mfma_f32_16x16x32_bf16 with the weights as the A operand
// (2 tiles of 16 output channels, one k-step of the 32 input channels per tap, fragments pre-packed on the host
// [tap][tile][lane][8]) and 16 pixels of one tile row as the B operand (lane l reads channels 8 (l >> 4) .. + 7 of
// pixel l & 15: one 16-B LDS read).  The accumulators of a lane are 8 channels of one pixel: folded BatchNorm +
// ReLU, the 1x1 (32 -> 3) as 8 products per lane summed over the 4 lane groups with two shuffles, then the blend.
using hiseg::bf16x8_t;
using hiseg::floatx4;
constexpr int kFT = 16, kFX = kFT + 4, kFH = kFT + 2;

__global__ void __launch_bounds__(256) refine_fused_kernel(
    const float* __restrict__ x, int H, int W, const float* __restrict__ e, const float* __restrict__ mnmx,
    const float* __restrict__ blend, const float* __restrict__ w1, const float* __restrict__ s1,
    const float* __restrict__ t1, const uint4* __restrict__ w2f, const float* __restrict__ s2,
    const float* __restrict__ t2, const float* __restrict__ w3, const float* __restrict__ b3,
    float* __restrict__ out) {
  __shared__ float sx[3][kFX][kFX];
  __shared__ __attribute__((aligned(16))) uint32_t sh1[kFH * kFH][16];   // 32 bf16 per position
  __shared__ float sw1[32 * 27];
  __shared__ float ss1[32], st1[32];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kFT, ty0 = blockIdx.y * kFT;
  const long long n = blockIdx.z, HW = (long long)H * W;
  const float* xs = x + n * 3 * HW;
  for (int i = tid; i < 3 * kFX * kFX; i += 256) {
    const int c = i / (kFX * kFX), r = i - c * kFX * kFX, yy = r / kFX, xx = r - yy * kFX;
    const int gy = ty0 + yy - 2, gx = tx0 + xx - 2;
    sx[c][yy][xx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xs[c * HW + (long long)gy * W + gx] : 0.f;
  }
  for (int i = tid; i < 32 * 27; i += 256) sw1[i] = w1[i];
  if (tid < 32) {
    ss1[tid] = s1[tid];
    st1[tid] = t1[tid];
  }
  __syncthreads();
  // conv1 + folded BatchNorm + ReLU at the halo-1 positions
  for (int p = tid; p < kFH * kFH; p += 256) {
    const int py = p / kFH, px = p - py * kFH;
    const int gy = ty0 + py - 1, gx = tx0 + px - 1;
    if (gy < 0 || gy >= H || gx < 0 || gx >= W) {
#pragma unroll
      for (int k = 0; k < 16; ++k) sh1[p][k] = 0u;
      continue;
    }
    float v[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) v[c * 9 + ky * 3 + kx] = sx[c][py + ky][px + kx];
    for (int co = 0; co < 32; co += 2) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        a0 += sw1[co * 27 + k] * v[k];
        a1 += sw1[(co + 1) * 27 + k] * v[k];
      }
      a0 = fmaxf(a0 * ss1[co] + st1[co], 0.f);
      a1 = fmaxf(a1 * ss1[co + 1] + st1[co + 1], 0.f);
      sh1[p][co >> 1] = hiseg::f2bf2(a0, a1);
    }
  }
  __syncthreads();
  // conv2 on MFMA
  const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, r = lane & 15;
  uint4 af[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) af[t][mt] = w2f[(t * 2 + mt) * 64 + lane];
  float sc[2][4], sf[2][4], wo[3][2][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ch = 16 * mt + 4 * g + q;
      sc[mt][q] = s2[ch];
      sf[mt][q] = t2[ch];
#pragma unroll
      for (int c = 0; c < 3; ++c) wo[c][mt][q] = w3[c * 32 + ch];
    }
  const float mn = mnmx[0], mx = mnmx[1], bw = blend[0];
  const bool flat = mx - mn < 1e-6f;
  const float D = mx - mn + 1e-6f;
#pragma unroll 1
  for (int pr = 0; pr < 4; ++pr) {
    const int py = wave * 4 + pr;
    floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ky = t / 3, kx = t - 3 * ky;
      const uint4 bf = *reinterpret_cast<const uint4*>(&sh1[(py + ky) * kFH + r + kx][4 * g]);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[t][mt]),
                                                          __builtin_bit_cast(bf16x8_t, bf), acc[mt], 0, 0, 0);
    }
    float rr[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float hv = fmaxf(acc[mt][q] * sc[mt][q] + sf[mt][q], 0.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) rr[c] += wo[c][mt][q] * hv;
      }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      rr[c] += __shfl_xor(rr[c], 16);
      rr[c] += __shfl_xor(rr[c], 32);
    }
    const int gy = ty0 + py, gx = tx0 + r;
    if (g == 0 && gy < H && gx < W) {
      const long long i = n * HW + (long long)gy * W + gx;
      const float E = flat ? 0.f : (e[i] - mn) / D;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        out[(n * 3 + c) * HW + (long long)gy * W + gx] = sx[c][py + 2][r + 2] + (bw * (rr[c] + b3[c])) * E;
    }
  }
}

int check_shape(const char* what, int N, int H, int W) {
  HISEG_REQUIRE(N >= 0 && H >= 0 && W >= 0, HISEG_ERR_BAD_ARG, "%s: negative size", what);
  HISEG_REQUIRE(H >= 2 && W >= 2, HISEG_ERR_BAD_ARG,
                "%s: H and W must be at least 2 (got %d x %d): the differences need two samples per axis", what, H,
                W);
  return HISEG_OK;
}

int check_cl(const char* what, const void* p, int dtype, int cs) {
  if (!p) return HISEG_OK;
  HISEG_REQUIRE(dtype == HISEG_F32 || dtype == HISEG_BF16, HISEG_ERR_BAD_DTYPE, "%s: channel-last dtype %d", what,
                dtype);
  HISEG_REQUIRE(cs >= 3, HISEG_ERR_BAD_SHAPE, "%s: channel stride %d < 3", what, cs);
  HISEG_REQUIRE(!((dtype == HISEG_BF16 && cs == 8) || (dtype == HISEG_F32 && cs == 4)) || al16(p),
                HISEG_ERR_BAD_SHAPE, "%s: channel-last buffer not 16-byte aligned", what);
  return HISEG_OK;
}

}  // namespace

extern "C" long long hiseg_edge_map_ws(int N, int H, int W) {
  if (N < 0 || H < 0 || W < 0) return 0;
  return 2LL * kMaxBlk;
}

extern "C" int hiseg_edge_map_fwd(const float* x, int N, int H, int W, float* e_raw, float* mnmx, float* probs,
                                  void* x_cl, int cl_dtype, int cl_cstride, float* ws, hiseg_stream_t stream) {
  if (int st = check_shape("edge_map_fwd", N, H, W)) return st;
  if (int st = check_cl("edge_map_fwd", x_cl, cl_dtype, cl_cstride)) return st;
  if (N == 0) return HISEG_OK;
  HISEG_REQUIRE(x && e_raw && mnmx && ws, HISEG_ERR_BAD_ARG, "edge_map_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int nb = grid_for((long long)N * H * W);
  edge_raw_kernel<<<nb, kT, 0, s>>>(x, N, H, W, e_raw, probs, x_cl, cl_dtype == HISEG_BF16, cl_cstride, ws);
  edge_minmax_kernel<<<1, kT, 0, s>>>(ws, nb, mnmx);
  return hiseg_check_launch("edge_map_fwd");
}

extern "C" int hiseg_boundary_blend_fwd(const float* x, const float* R, int r_cstride, const float* e_raw,
                                        const float* mnmx, const float* blend, int N, int H, int W, float* out,
                                        float* E_out, hiseg_stream_t stream) {
  if (int st = check_shape("boundary_blend_fwd", N, H, W)) return st;
  if (N == 0) return HISEG_OK;
  HISEG_REQUIRE(x && R && e_raw && mnmx && blend && out, HISEG_ERR_BAD_ARG, "boundary_blend_fwd: null pointer");
  HISEG_REQUIRE(r_cstride >= 3, HISEG_ERR_BAD_SHAPE, "boundary_blend_fwd: channel stride %d < 3", r_cstride);
  blend_fwd_kernel<<<grid_for((long long)N * H * W), kT, 0, (hipStream_t)stream>>>(x, R, r_cstride, e_raw, mnmx,
                                                                                   blend, N, H, W, out, E_out);
  return hiseg_check_launch("boundary_blend_fwd");
}

extern "C" long long hiseg_boundary_bwd_ws(int N, int H, int W) {
  if (N < 0 || H < 0 || W < 0) return 0;
  return 16 + 10LL * kMaxBlk + 7LL * N * H * W;
}

extern "C" int hiseg_boundary_blend_bwd(const float* g, const float* R, int r_cstride, const float* e_raw,
                                        const float* mnmx, const float* blend, int N, int H, int W, float* dR,
                                        int dr_cstride, float* dblend, float* ws, hiseg_stream_t stream) {
  if (int st = check_shape("boundary_blend_bwd", N, H, W)) return st;
  if (N == 0) return HISEG_OK;
  HISEG_REQUIRE(g && R && e_raw && mnmx && blend && dR && ws, HISEG_ERR_BAD_ARG, "boundary_blend_bwd: null pointer");
  HISEG_REQUIRE(r_cstride >= 3 && dr_cstride >= 3, HISEG_ERR_BAD_SHAPE, "boundary_blend_bwd: channel stride < 3");
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, HISEG_ERR_BAD_SHAPE, "boundary_blend_bwd: ws alignment");
  hipStream_t s = (hipStream_t)stream;
  const long long P = (long long)N * H * W;
  const BwdWs w = bwd_ws(ws, P);
  const int nb = grid_for(P);
  blend_bwd_kernel<<<nb, kT, 0, s>>>(g, R, r_cstride, e_raw, mnmx, blend, N, H, W, dR, dr_cstride, w.dE, w.part);
  blend_sums_kernel<<<1, kT, 0, s>>>(w.part, nb, w.sums, dblend);
  return hiseg_check_launch("boundary_blend_bwd");
}

extern "C" int hiseg_edge_map_bwd(const float* g, const void* g_cl, int cl_dtype, int cl_cstride, const float* probs,
                                  const float* e_raw, const float* mnmx, int N, int H, int W, float* ws, float* dx,
                                  hiseg_stream_t stream) {
  if (int st = check_shape("edge_map_bwd", N, H, W)) return st;
  if (int st = check_cl("edge_map_bwd", g_cl, cl_dtype, cl_cstride)) return st;
  if (N == 0) return HISEG_OK;
  HISEG_REQUIRE(g && probs && e_raw && mnmx && ws && dx, HISEG_ERR_BAD_ARG, "edge_map_bwd: null pointer");
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, HISEG_ERR_BAD_SHAPE, "edge_map_bwd: ws alignment");
  hipStream_t s = (hipStream_t)stream;
  const long long P = (long long)N * H * W;
  const BwdWs w = bwd_ws(ws, P);
  const int nb = grid_for(P);
  edge_bwd_a_kernel<<<nb, kT, 0, s>>>(probs, e_raw, mnmx, N, H, W, w.sums, w.dE, w.A);
  edge_bwd_b_kernel<<<nb, kT, 0, s>>>(g, g_cl, cl_dtype == HISEG_BF16, cl_cstride, probs, mnmx, N, H, W, w.A, dx);
  return hiseg_check_launch("edge_map_bwd");
}

extern "C" long long hiseg_active_contour_ws(int N, int H, int W) {
  if (N < 0 || H < 0 || W < 0) return 0;
  return 8 + 8LL * kMaxBlk + (long long)N * H * W;
}

extern "C" int hiseg_active_contour_fwd(const float* pred, int N, int H, int W, float* ws, float* out,
                                        hiseg_stream_t stream) {
  if (int st = check_shape("active_contour_fwd", N, H, W)) return st;
  HISEG_REQUIRE(N >= 1, HISEG_ERR_BAD_ARG, "active_contour_fwd: empty batch");
  HISEG_REQUIRE(pred && ws && out, HISEG_ERR_BAD_ARG, "active_contour_fwd: null pointer");
  HISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, HISEG_ERR_BAD_SHAPE, "active_contour_fwd: ws alignment");
  hipStream_t s = (hipStream_t)stream;
  const long long HW = (long long)H * W;
  const int nb = grid_for(N * HW);
  ac_prob_kernel<<<nb, kT, 0, s>>>(pred, N, HW, ac_q(ws));
  ac_sum_kernel<<<nb, kT, 0, s>>>(ac_q(ws), N, H, W, ac_part(ws));
  ac_final_kernel<<<1, kT, 0, s>>>(ac_part(ws), nb, N, H, W, ws, out);
  return hiseg_check_launch("active_contour_fwd");
}

extern "C" int hiseg_active_contour_bwd(const float* pred, int N, int H, int W, const float* ws, const float* gscale,
                                        float* dpred, hiseg_stream_t stream) {
  if (int st = check_shape("active_contour_bwd", N, H, W)) return st;
  HISEG_REQUIRE(N >= 1, HISEG_ERR_BAD_ARG, "active_contour_bwd: empty batch");
  HISEG_REQUIRE(pred && ws && gscale && dpred, HISEG_ERR_BAD_ARG, "active_contour_bwd: null pointer");
  float* w = const_cast<float*>(ws);
  ac_bwd_kernel<<<grid_for((long long)N * H * W), kT, 0, (hipStream_t)stream>>>(pred, ac_q(w), w, gscale, N, H, W,
                                                                                dpred);
  return hiseg_check_launch("active_contour_bwd");
}

extern "C" int hiseg_boundary_refine_fused(const float* x, int N, int H, int W, const float* e_raw, const float* mnmx,
                                           const float* blend, const float* w1, const float* scale1,
                                           const float* shift1, const void* w2_frag, const float* scale2,
                                           const float* shift2, const float* w3, const float* b3, float* out,
                                           hiseg_stream_t stream) {
  if (int st = check_shape("boundary_refine_fused", N, H, W)) return st;
  if (N == 0) return HISEG_OK;
  HISEG_REQUIRE(x && e_raw && mnmx && blend && w1 && scale1 && shift1 && w2_frag && scale2 && shift2 && w3 && b3 && out,
                HISEG_ERR_BAD_ARG, "boundary_refine_fused: null pointer");
  HISEG_REQUIRE(al16(w2_frag), HISEG_ERR_BAD_SHAPE, "boundary_refine_fused: w2_frag not 16-byte aligned");
  HISEG_REQUIRE(N <= 65535 && (H + kFT - 1) / kFT <= 65535, HISEG_ERR_BAD_SHAPE,
                "boundary_refine_fused: grid too large (N %d, H %d)", N, H);
  const dim3 grid((W + kFT - 1) / kFT, (H + kFT - 1) / kFT, N);
  refine_fused_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, H, W, e_raw, mnmx, blend, w1, scale1, shift1,
                                                             reinterpret_cast<const uint4*>(w2_frag), scale2, shift2,
                                                             w3, b3, out);
  return hiseg_check_launch("boundary_refine_fused");
}
