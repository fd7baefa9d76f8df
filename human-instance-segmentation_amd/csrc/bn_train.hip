#include <cstdlib>
// Train-mode BatchNorm of the ROI path (gfx950): statistics, finalize, apply and backward, each as a scalar and a
// 16-B-chunk kernel.  HBM-streaming passes over NHWC activations: f32 arithmetic, storage in the compute dtype,
// statistics as deterministic per-split partials (no atomics) combined in double precision by the finalize kernels.
// hiseg_bn_apply also is LayerNorm2d's forward apply (per_sample tables; ln_train.hip holds the rest of LayerNorm2d).
#include "train_norm.h"

namespace hiseg {

constexpr int kBnSplits = 1024;  // pixel splits of the statistics passes (4 blocks per CU)

// Pixel range of split s.
__device__ __forceinline__ void split_range(long long P, int s, int S, long long& b, long long& e) {
  b = P * s / S;
  e = P * (s + 1) / S;
}

// ---------------------------------------------------------------------------------------- stats
// Block layout: CT = min(C, 256) channel lanes x R = 256/CT pixel rows; channel block blockIdx.y.
template <typename T>
__global__ void __launch_bounds__(256) bn_stats_kernel(const void* z, long long P, int C, int cs, int coff,
                                                       float* partial) {
  __shared__ float sh_n[256], sh_m[256], sh_q[256];
  const int CT = C < 256 ? C : 256;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int c = blockIdx.y * 256 + cl;
  long long b, e;
  split_range(P, blockIdx.x, gridDim.x, b, e);
  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (r < R && c < C) {
    for (long long p = b + r; p < e; p += R) {
      const float x = ld<T>(z, p * cs + coff + c);
      n += 1.f;
      const float d = x - mean;
      mean += d / n;
      m2 += d * (x - mean);
    }
  }
  sh_n[t] = n; sh_m[t] = mean; sh_q[t] = m2;
  __syncthreads();
  if (r == 0 && c < C) {
    for (int rr = 1; rr < R; ++rr) {
      const int o = rr * CT + cl;
      const float nb = sh_n[o];
      if (nb == 0.f) continue;
      const float na = n, nt = na + nb;
      const float d = sh_m[o] - mean;
      mean += d * (nb / nt);
      m2 += sh_q[o] + d * d * (na * nb / nt);
      n = nt;
    }
    float* out = partial + (long long)blockIdx.x * 3 * C;
    out[c] = n; out[C + c] = mean; out[2 * C + c] = m2;
  }
}

// ---------------------------------------------------------------------------------------- apply
template <typename T>
__global__ void __launch_bounds__(256) bn_apply_kernel(hiseg_bn_apply_desc d) {
  const long long n = d.P * d.C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long p = i / d.C;
    const int c = (int)(i - p * d.C);
    const long long tc = d.per_sample ? (p / d.HW) * d.C + c : c;
    float v = ld<T>(d.z, p * d.z_cstride + d.z_coff + c) * d.scale[tc] + d.shift[tc];
    if (d.residual) v += ld<T>(d.residual, p * d.r_cstride + d.r_coff + c);
    v = apply_act(v, d.act, d.act_beta);
    if (d.chan_mul) v *= d.chan_mul[(p / d.HW) * d.C + c];
    st<T>(d.y, p * d.y_cstride + d.y_coff + c, v);
  }
}

// ---------------------------------------------------------------------------------------- backward
__device__ __forceinline__ float silu_grad_pre(const hiseg_bn_bwd_desc& d, float z, int c) {
  const float v = (z - d.mean[c]) * d.invstd[c] * (d.gamma ? d.gamma[c] : 1.f) + (d.beta ? d.beta[c] : 0.f);
  const float s = 1.f / (1.f + expf(-v));
  return s * (1.f + v * (1.f - s));
}

// The derivative is taken at the forward's own pre-activation z*fwd_scale + fwd_shift (+ residual) when the
// folded affine is given and the activation needs it (smooth ones; ReLU after a residual add with the residual).
__host__ __device__ __forceinline__ bool bn_pre_path(const hiseg_bn_bwd_desc& d) {
  return d.fwd_scale && (act_smooth(d.act) || (d.act == HISEG_ACT_RELU && (!d.dres || d.residual)));
}

template <typename T>
__device__ __forceinline__ float bn_g(const hiseg_bn_bwd_desc& d, long long p, int c) {
  float g = ld<T>(d.dy, p * d.dy_cstride + d.dy_coff + c);
  if (d.chan_mul) g *= d.chan_mul[(p / d.HW) * d.C + c];
  if (bn_pre_path(d)) {
    float v = ld<T>(d.z, p * d.z_cstride + d.z_coff + c) * d.fwd_scale[c] + d.fwd_shift[c];
    if (d.residual) v += ld<T>(d.residual, p * d.r_cstride + d.r_coff + c);
    g *= act_grad_pre(v, d.act, d.act_beta);
  } else if (d.act == HISEG_ACT_SILU) g *= silu_grad_pre(d, ld<T>(d.z, p * d.z_cstride + d.z_coff + c), c);
  else if (d.act != HISEG_ACT_NONE) g *= act_grad(ld<T>(d.y, p * d.y_cstride + d.y_coff + c), d.act);
  return g;
}

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(hiseg_bn_bwd_desc d) {
  __shared__ float sa[256], sb[256], sc[256];
  const int C = d.C;
  const int CT = C < 256 ? C : 256;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int c = blockIdx.y * 256 + cl;
  long long b, e;
  split_range(d.P, blockIdx.x, gridDim.x, b, e);
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (r < R && c < C) {
    const float mu = d.mean[c], inv = d.invstd[c];
    for (long long p = b + r; p < e; p += R) {
      const float g = bn_g<T>(d, p, c);
      const float xh = (ld<T>(d.z, p * d.z_cstride + d.z_coff + c) - mu) * inv;
      s1 += g; s2 += g * xh; s3 += xh;
    }
  }
  sa[t] = s1; sb[t] = s2; sc[t] = s3;
  __syncthreads();
  if (r == 0 && c < C) {
    for (int rr = 1; rr < R; ++rr) {
      s1 += sa[rr * CT + cl]; s2 += sb[rr * CT + cl]; s3 += sc[rr * CT + cl];
    }
    float* out = d.partial + (long long)blockIdx.x * 3 * C;
    out[c] = s1; out[C + c] = s2; out[2 * C + c] = s3;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(hiseg_bn_bwd_desc d, int S) {
  const int C = d.C;
  const float* coef = d.partial + (long long)S * 3 * C;
  const long long n = d.P * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long p = i / C;
    const int c = (int)(i - p * C);
    const float g = bn_g<T>(d, p, c);
    const float xh = (ld<T>(d.z, p * d.z_cstride + d.z_coff + c) - d.mean[c]) * d.invstd[c];
    st<T>(d.dz, p * d.dz_cstride + d.dz_coff + c, coef[c] * (g - coef[C + c] - xh * coef[2 * C + c]));
    if (d.dres) {
      const long long o = p * d.dres_cstride + d.dres_coff + c;
      st<T>(d.dres, o, d.dres_accumulate ? ld<T>(d.dres, o) + g : g);
    }
  }
}

// ---------------------------------------------------------------------------------------- vectorised
// The same passes with one 16-B chunk (8 bf16 / 4 f32 channels) per thread per pixel: a wavefront
// reads 64 x 16 B = 1 KiB per load instruction, pixel rows of a block are contiguous in HBM (NHWC),
// so every pass streams at HBM rate.  Block = CT chunk lanes x R pixel rows (CT = min(C/VEC, 256)).
// Used whenever channels, strides and offsets are multiples of the chunk (all hiseg activations).
template <typename T>
__global__ void __launch_bounds__(256) bn_stats_vec_kernel(const void* z, long long P, int C, int cs, int coff,
                                                           float* partial) {
  constexpr int V = Chunk<T>::N;
  __shared__ float sh[256 * (2 * V + 1)];
  const int NCH = C / V;
  const int CT = NCH < 256 ? NCH : 256;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int ch = blockIdx.y * 256 + cl;
  const bool live = r < R && ch < NCH;
  long long b, e;
  split_range(P, blockIdx.x, gridDim.x, b, e);
  float n = 0.f, mean[V], m2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) mean[k] = m2[k] = 0.f;
  if (live) {
    // four pixels' loads in flight before their Welford updates (the updates are a dependent chain; the loads are
    // not): the small deep layers give each thread tens of pixels at L2 / HBM latency.  Same update order as one by one.
    auto upd = [&](const float* x) __attribute__((always_inline)) {
      n += 1.f;
      const float rn = 1.f / n;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float d = x[k] - mean[k];
        mean[k] += d * rn;
        m2[k] += d * (x[k] - mean[k]);
      }
    };
    long long p = b + r;
    for (; p + 3 * R < e; p += 4 * R) {
      float x0[V], x1[V], x2[V], x3[V];
      ldv<T>(z, p * cs + coff + ch * V, x0);
      ldv<T>(z, (p + R) * cs + coff + ch * V, x1);
      ldv<T>(z, (p + 2 * R) * cs + coff + ch * V, x2);
      ldv<T>(z, (p + 3 * R) * cs + coff + ch * V, x3);
      upd(x0); upd(x1); upd(x2); upd(x3);
    }
    for (; p < e; p += R) {
      float x[V];
      ldv<T>(z, p * cs + coff + ch * V, x);
      upd(x);
    }
  }
  float* my = sh + t * (2 * V + 1);
  my[0] = n;
#pragma unroll
  for (int k = 0; k < V; ++k) { my[1 + k] = mean[k]; my[1 + V + k] = m2[k]; }
  // pairwise (tree) merge of the R pixel rows, fixed order: the one-thread walk over R - 1 rows was a dependent chain
  // of divisions (R = 128 for the 16-channel decoder layers: 31 us per 26 MB layer)
  for (int step = 1; step < R; step <<= 1) {
    __syncthreads();
    if (r % (2 * step) == 0 && r + step < R && ch < NCH) {
      const float* o = sh + ((r + step) * CT + cl) * (2 * V + 1);
      const float nb = o[0];
      if (nb != 0.f) {
        const float na = n, nt = na + nb;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float d = o[1 + k] - mean[k];
          mean[k] += d * (nb / nt);
          m2[k] += o[1 + V + k] + d * d * (na * nb / nt);
        }
        n = nt;
        my[0] = n;
#pragma unroll
        for (int k = 0; k < V; ++k) { my[1 + k] = mean[k]; my[1 + V + k] = m2[k]; }
      }
    }
  }
  if (r == 0 && ch < NCH) {
    float* out = partial + (long long)blockIdx.x * 3 * C + ch * V;
#pragma unroll
    for (int k = 0; k < V; ++k) { out[k] = n; out[C + k] = mean[k]; out[2 * C + k] = m2[k]; }
  }
}

// Split groups of a large split count (the conv epilogue's fused statistics: one split per (pixel tile, wave), 12 288
// for a 256-ROI 64x48 layer): one block per (64 channels, KPRE consecutive splits), 4 rows x 64 channel lanes
// (coalesced loads across the lanes).  Row r sums every 4th split of the group as (n, sum n mean, sum M2 + n mean^2)
// in double -- no division in the loop -- and the 4 rows' sums are added in a fixed order; the group's (n, mean, M2)
// overwrites its own first split row (read by this block only), so bn_finalize_par_kernel merges S / KPRE rows at a
// stride of KPRE rows.  (One block per channel reading S strided rows: 85 us per 256-channel layer on 12 288 splits;
// this kernel with a Chan merge per split: 17 us.)
constexpr int KPRE = 64;
__global__ void __launch_bounds__(256) bn_premerge_kernel(float* partial, int S, int C) {
  __shared__ double sn[4][64], s1[4][64], s2[4][64];
  const int t = threadIdx.x, l = t & 63, r = t >> 6;
  const int c = blockIdx.x * 64 + l;
  const int s0 = blockIdx.y * KPRE;
  double n = 0, a = 0, b = 0;
  if (c < C) {
#pragma unroll 4
    for (int i = r; i < KPRE; i += 4) {
      if (s0 + i >= S) break;
      const float* p = partial + (long long)(s0 + i) * 3 * C;
      const double ni = p[c], mi = p[C + c], qi = p[2 * C + c];
      n += ni;
      a = fma(ni, mi, a);
      b += qi + ni * mi * mi;
    }
  }
  sn[r][l] = n; s1[r][l] = a; s2[r][l] = b;
  __syncthreads();
  if (r == 0 && c < C) {
    n = (sn[0][l] + sn[1][l]) + (sn[2][l] + sn[3][l]);
    a = (s1[0][l] + s1[1][l]) + (s1[2][l] + s1[3][l]);
    b = (s2[0][l] + s2[1][l]) + (s2[2][l] + s2[3][l]);
    const double mean = n > 0 ? a / n : 0.0;
    const double m2 = n > 0 ? fmax(b - a * mean, 0.0) : 0.0;
    float* o = partial + (long long)s0 * 3 * C;
    o[c] = (float)n;
    o[C + c] = (float)mean;
    o[2 * C + c] = (float)m2;
  }
}

// One block per channel: 256 threads merge the S split partials (rows `rs` floats apart; Chan, double), tree-combined
// in LDS.
__global__ void __launch_bounds__(256) bn_finalize_par_kernel(const float* partial, int S, int C, long long P,
                                                              const float* gamma, const float* beta, float eps,
                                                              float momentum, float* rm, float* rv, float* mean_o,
                                                              float* invstd_o, float* scale, float* shift,
                                                              long long rs) {
  __shared__ double sn[256], sm[256], sq[256];
  const int c = blockIdx.x, t = threadIdx.x;
  double n = 0, mean = 0, m2 = 0;
  // a thread's (up to four) partials loaded before its merges: one round of load latency instead of four
  for (int s0 = t; s0 < S; s0 += 1024) {
    float pn[4], pm[4], pq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = s0 + 256 * u;
      const float* p = partial + (long long)(s < S ? s : 0) * rs;
      pn[u] = s < S ? p[c] : 0.f;
      pm[u] = p[C + c];
      pq[u] = p[2 * C + c];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double nb = pn[u];
      if (nb == 0) continue;
      const double d = pm[u] - mean, nt = n + nb;
      mean += d * nb / nt;
      m2 += pq[u] + d * d * n * nb / nt;
      n = nt;
    }
  }
  sn[t] = n; sm[t] = mean; sq[t] = m2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const double na = sn[t], nb = sn[t + w];
      if (nb > 0) {
        const double nt = na + nb, d = sm[t + w] - sm[t];
        sm[t] += d * nb / nt;
        sq[t] += sq[t + w] + d * d * na * nb / nt;
        sn[t] = nt;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const double var = sq[0] / sn[0];
    const double inv = 1.0 / sqrt(var + (double)eps);
    const double mu = sm[0];
    const float g = gamma ? gamma[c] : 1.f, bb = beta ? beta[c] : 0.f;
    mean_o[c] = (float)mu;
    invstd_o[c] = (float)inv;
    scale[c] = (float)(g * inv);
    shift[c] = (float)(bb - mu * g * inv);
    if (rm) rm[c] = (float)((1.0 - momentum) * rm[c] + momentum * mu);
    if (rv) rv[c] = (float)((1.0 - momentum) * rv[c] + momentum * (P > 1 ? var * (double)P / (double)(P - 1) : var));
  }
}

// The same merge as 16 channel lanes x 16 split rows per block (round 6): row r sums splits r, r + 16, ... of its
// channel as (n, sum n mean, sum M2 + n mean^2) in double, four splits' loads in flight, no division in the loop
// (bn_premerge_kernel's form); the 16 rows are added in a fixed order.  C / 16 blocks instead of C: the per-channel
// kernel's 256-thread block and eight-level double Chan tree per channel cost ~7 us a call whatever S, on ~58 calls
// of the distillation student's forward.  Within f32 rounding of the Chan merge (test_bn_finalize_n_matches_f64_merge).
__global__ void __launch_bounds__(256) bn_finalize_rows_kernel(const float* partial, int S, int C, long long P,
                                                               const float* gamma, const float* beta, float eps,
                                                               float momentum, float* rm, float* rv, float* mean_o,
                                                               float* invstd_o, float* scale, float* shift,
                                                               long long rs) {
  __shared__ double sn[16][16], sa[16][16], sb[16][16];
  const int l = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + l;
  double n = 0, a = 0, b = 0;
  if (c < C) {
    int s = r;
    for (; s + 48 < S; s += 64) {
      float pn[4], pm[4], pq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* p = partial + (long long)(s + 16 * u) * rs;
        pn[u] = p[c];
        pm[u] = p[C + c];
        pq[u] = p[2 * C + c];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double ni = pn[u], mi = pm[u];
        n += ni;
        a = fma(ni, mi, a);
        b += (double)pq[u] + ni * mi * mi;
      }
    }
    for (; s < S; s += 16) {
      const float* p = partial + (long long)s * rs;
      const double ni = p[c], mi = p[C + c];
      n += ni;
      a = fma(ni, mi, a);
      b += (double)p[2 * C + c] + ni * mi * mi;
    }
  }
  sn[r][l] = n; sa[r][l] = a; sb[r][l] = b;
  __syncthreads();
  if (r != 0 || c >= C) return;
  for (int q = 1; q < 16; ++q) { n += sn[q][l]; a += sa[q][l]; b += sb[q][l]; }
  const double mu = n > 0 ? a / n : 0.0;
  const double var = n > 0 ? fmax(b - a * mu, 0.0) / n : 0.0;
  const double inv = 1.0 / sqrt(var + (double)eps);
  const float g = gamma ? gamma[c] : 1.f, bb = beta ? beta[c] : 0.f;
  mean_o[c] = (float)mu;
  invstd_o[c] = (float)inv;
  scale[c] = (float)(g * inv);
  shift[c] = (float)(bb - mu * g * inv);
  if (rm) rm[c] = (float)((1.0 - momentum) * rm[c] + momentum * mu);
  if (rv) rv[c] = (float)((1.0 - momentum) * rv[c] + momentum * (P > 1 ? var * (double)P / (double)(P - 1) : var));
}

// Element-wise passes: block = CT chunk lanes x R pixel rows (as the reductions), blocks stride over pixel
// rows; 32-bit pixel indices (P < 2^31, checked on the host), no per-element 64-bit division.
template <typename T, int U = 1>
__global__ void __launch_bounds__(256) bn_apply_vec_kernel(hiseg_bn_apply_desc d) {
  constexpr int V = Chunk<T>::N;
  const int NCH = d.C / V;
  const int CT = NCH < 256 ? NCH : 256;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int ch = blockIdx.y * 256 + cl;
  if (r >= R || ch >= NCH) return;
  const int c = ch * V;
  const int P = (int)d.P;
  float sc[V], sf[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { sc[k] = d.per_sample ? 0.f : d.scale[c + k]; sf[k] = d.per_sample ? 0.f : d.shift[c + k]; }
  // U pixels per iteration, their loads issued together (the pixels and the per-element arithmetic are U = 1's)
  const int stride = gridDim.x * R;
  for (int p0 = blockIdx.x * R + r; p0 < P; p0 += U * stride) {
    float v[U][V], rr[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * stride;
      if (p >= P) continue;
      ldv<T>(d.z, (long long)p * d.z_cstride + d.z_coff + c, v[u]);
      if (d.residual) ldv<T>(d.residual, (long long)p * d.r_cstride + d.r_coff + c, rr[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * stride;
      if (p >= P) continue;
      const float* cm = d.chan_mul ? d.chan_mul + (long long)(p / d.HW) * d.C + c : nullptr;
      if (d.per_sample) {   // LayerNorm2d: the sample's folded tables
        const long long tb = (long long)(p / d.HW) * d.C + c;
#pragma unroll
        for (int k = 0; k < V; ++k) { sc[k] = d.scale[tb + k]; sf[k] = d.shift[tb + k]; }
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float x = v[u][k] * sc[k] + sf[k];
        if (d.residual) x += rr[u][k];
        x = apply_act(x, d.act, d.act_beta);
        if (cm) x *= cm[k];
        v[u][k] = x;
      }
      stv<T>(d.y, (long long)p * d.y_cstride + d.y_coff + c, v[u]);
    }
  }
}

// How the backward pass gets act'(.) (bn_bwd_mode on the host; a template argument so the per-element loop
// carries no activation switch and the per-channel tables live in registers, loaded once per thread):
//   kGNone  identity;  kGY  act'(y) from the stored output (ReLU / Sigmoid, no folded affine given);
//   kGReLU  ReLU mask at the forward's pre-activation z*fwd_scale + fwd_shift (+ residual);
//   kGPre   any activation's derivative at that pre-activation (smooth ones; SiLU without the forward's tables
//           folds them here from mean / invstd / gamma / beta).
enum { kGNone = 0, kGY = 1, kGReLU = 2, kGPre = 3 };

__host__ __device__ __forceinline__ int bn_bwd_mode(const hiseg_bn_bwd_desc& d) {
  if (d.act == HISEG_ACT_NONE) return kGNone;
  if (bn_pre_path(d)) return d.act == HISEG_ACT_RELU ? kGReLU : kGPre;
  if (d.act == HISEG_ACT_SILU) return kGPre;
  return kGY;
}

// the pre-activation's per-channel affine of chunk c (modes kGReLU / kGPre)
template <int V>
__device__ __forceinline__ void bn_pre_tables(const hiseg_bn_bwd_desc& d, int c, float* fs, float* fh) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if (d.fwd_scale) {
      fs[k] = d.fwd_scale[c + k];
      fh[k] = d.fwd_shift[c + k];
    } else {
      const float kk = d.invstd[c + k] * (d.gamma ? d.gamma[c + k] : 1.f);
      fs[k] = kk;
      fh[k] = (d.beta ? d.beta[c + k] : 0.f) - d.mean[c + k] * kk;
    }
  }
}

// a * b rounded to f32: not a candidate for fusion into an add or subtract that consumes it
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// g = dy (* chan_mul) * act'(.) for one 16-B chunk; z = the chunk's pre-BN values (already loaded).  The products
// are mul_rounded, so dz, dres and the sums are all built from one rounded g whatever code surrounds the call: the
// U = 1 instance of bn_bwd_apply_vec_kernel used to fuse g's last multiply into g - sum(g)/P while the U = 2 instance,
// with the multiply in its load loop (another basic block), could not, and their f32 dz were one rounding apart for
// sigmoid / SiLU / GELU / Swish.
template <typename T, int MODE>
__device__ __forceinline__ void bn_gv(const hiseg_bn_bwd_desc& d, int p, int c, float* g, const float* z,
                                      const float* fs, const float* fh) {
  constexpr int V = Chunk<T>::N;
  ldv<T>(d.dy, (long long)p * d.dy_cstride + d.dy_coff + c, g);
  if (d.chan_mul) {
    const float* cm = d.chan_mul + (long long)(p / d.HW) * d.C + c;
#pragma unroll
    for (int k = 0; k < V; ++k) g[k] = mul_rounded(g[k], cm[k]);
  }
  if constexpr (MODE == kGReLU || MODE == kGPre) {
    float rr[V];
    if (d.residual) ldv<T>(d.residual, (long long)p * d.r_cstride + d.r_coff + c, rr);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float v = z[k] * fs[k] + fh[k];
      if (d.residual) v += rr[k];
      if constexpr (MODE == kGReLU) g[k] = v > 0.f ? g[k] : 0.f;
      else g[k] = mul_rounded(g[k], act_grad_pre(v, d.act, d.act_beta));
    }
  } else if constexpr (MODE == kGY) {
    float y[V];
    ldv<T>(d.y, (long long)p * d.y_cstride + d.y_coff + c, y);
#pragma unroll
    for (int k = 0; k < V; ++k) g[k] = mul_rounded(g[k], act_grad(y[k], d.act));
  }
}

template <typename T, int MODE>
__global__ void __launch_bounds__(256) bn_bwd_reduce_vec_kernel(hiseg_bn_bwd_desc d) {
  constexpr int V = Chunk<T>::N;
  __shared__ float sh[256 * 3 * V];
  const int C = d.C;
  const int NCH = C / V;
  const int CT = NCH < 256 ? NCH : 256;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int ch = blockIdx.y * 256 + cl;
  const int c = ch * V;
  long long b, e;
  split_range(d.P, blockIdx.x, gridDim.x, b, e);
  float s1[V], s2[V], s3[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s1[k] = s2[k] = s3[k] = 0.f;
  if (r < R && ch < NCH) {
    float mu[V], inv[V], fs[V], fh[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { mu[k] = d.mean[c + k]; inv[k] = d.invstd[c + k]; }
    if constexpr (MODE == kGReLU || MODE == kGPre) bn_pre_tables<V>(d, c, fs, fh);
    // (a four-way unroll here measured slower: 75 -> 91 and 103 -> 146 us on the train step's 256-channel layers)
    for (int p = (int)b + r; p < (int)e; p += R) {
      float g[V], z[V];
      ldv<T>(d.z, (long long)p * d.z_cstride + d.z_coff + c, z);
      bn_gv<T, MODE>(d, p, c, g, z, fs, fh);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float xh = (z[k] - mu[k]) * inv[k];
        s1[k] += g[k]; s2[k] += g[k] * xh; s3[k] += xh;
      }
    }
  }
  float* my = sh + t * 3 * V;
#pragma unroll
  for (int k = 0; k < V; ++k) { my[k] = s1[k]; my[V + k] = s2[k]; my[2 * V + k] = s3[k]; }
  // pairwise (tree) sum of the R pixel rows, fixed order (was one thread walking R - 1 rows)
  for (int step = 1; step < R; step <<= 1) {
    __syncthreads();
    if (r % (2 * step) == 0 && r + step < R && ch < NCH) {
      const float* o = sh + ((r + step) * CT + cl) * 3 * V;
#pragma unroll
      for (int k = 0; k < V; ++k) { s1[k] += o[k]; s2[k] += o[V + k]; s3[k] += o[2 * V + k]; }
#pragma unroll
      for (int k = 0; k < V; ++k) { my[k] = s1[k]; my[V + k] = s2[k]; my[2 * V + k] = s3[k]; }
    }
  }
  if (r == 0 && ch < NCH) {
    float* out = d.partial + (long long)blockIdx.x * 3 * C + c;
#pragma unroll
    for (int k = 0; k < V; ++k) { out[k] = s1[k]; out[C + k] = s2[k]; out[2 * C + k] = s3[k]; }
  }
}

__global__ void __launch_bounds__(256) bn_bwd_finalize_par_kernel(hiseg_bn_bwd_desc d, int S) {
  __shared__ double a1[256], a2[256], a3[256];
  const int c = blockIdx.x, t = threadIdx.x, C = d.C;
  double s1 = 0, s2 = 0, s3 = 0;
  for (int s0 = t; s0 < S; s0 += 1024) {   // (up to four partials' loads in flight, then the sums in order)
    float v1[4], v2[4], v3[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = s0 + 256 * u;
      const float* p = d.partial + (long long)(s < S ? s : 0) * 3 * C;
      v1[u] = s < S ? p[c] : 0.f;
      v2[u] = s < S ? p[C + c] : 0.f;
      v3[u] = s < S ? p[2 * C + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { s1 += v1[u]; s2 += v2[u]; s3 += v3[u]; }
  }
  a1[t] = s1; a2[t] = s2; a3[t] = s3;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) { a1[t] += a1[t + w]; a2[t] += a2[t + w]; a3[t] += a3[t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    s1 = a1[0]; s2 = a2[0]; s3 = a3[0];
    const double P = (double)d.P;
    const double k = (d.gamma ? d.gamma[c] : 1.0) * d.invstd[c];
    float* coef = d.partial + (long long)S * 3 * C;
    coef[c] = (float)k;
    coef[C + c] = (float)(s1 / P);
    coef[2 * C + c] = (float)(s2 / P);
    if (d.dgamma) d.dgamma[c] = (float)(d.accumulate_params ? d.dgamma[c] + s2 : s2);
    if (d.dbeta) d.dbeta[c] = (float)(d.accumulate_params ? d.dbeta[c] + s1 : s1);
    if (d.dconv_bias) {
      const double sdz = k * (s1 - P * (s1 / P) - s3 * (s2 / P));
      d.dconv_bias[c] = (float)(d.accumulate_params ? d.dconv_bias[c] + sdz : sdz);
    }
  }
}

template <typename T, int MODE, int U = 1>
__global__ void __launch_bounds__(256) bn_bwd_apply_vec_kernel(hiseg_bn_bwd_desc d, int S) {
  constexpr int V = Chunk<T>::N;
  const int C = d.C;
  const int NCH = C / V;
  const int CT = NCH < 256 ? NCH : 256;
  const int R = 256 / CT;
  const int t = threadIdx.x;
  const int cl = t % CT, r = t / CT;
  const int ch = blockIdx.y * 256 + cl;
  if (r >= R || ch >= NCH) return;
  const int c = ch * V;
  const float* coef = d.partial + (long long)S * 3 * C;
  float k0[V], k1[V], k2[V], mu[V], inv[V], fs[V], fh[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    k0[k] = coef[c + k]; k1[k] = coef[C + c + k]; k2[k] = coef[2 * C + c + k];
    mu[k] = d.mean[c + k]; inv[k] = d.invstd[c + k];
  }
  if constexpr (MODE == kGReLU || MODE == kGPre) bn_pre_tables<V>(d, c, fs, fh);
  const int P = (int)d.P;
  const int stride = gridDim.x * R;
  for (int p0 = blockIdx.x * R + r; p0 < P; p0 += U * stride) {
    float g[U][V], z[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {   // U pixels' loads together (bn_gv loads dy / y / residual)
      const int p = p0 + u * stride;
      if (p >= P) continue;
      ldv<T>(d.z, (long long)p * d.z_cstride + d.z_coff + c, z[u]);
      bn_gv<T, MODE>(d, p, c, g[u], z[u], fs, fh);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * stride;
      if (p >= P) continue;
      float o[V];
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = k0[k] * (g[u][k] - k1[k] - (z[u][k] - mu[k]) * inv[k] * k2[k]);
      stv<T>(d.dz, (long long)p * d.dz_cstride + d.dz_coff + c, o);
      if (d.dres) {
        const long long off = (long long)p * d.dres_cstride + d.dres_coff + c;
        if (d.dres_accumulate) {
          float rv[V];
          ldv<T>(d.dres, off, rv);
#pragma unroll
          for (int k = 0; k < V; ++k) g[u][k] += rv[k];
        }
        stv<T>(d.dres, off, g[u]);
      }
    }
  }
}
}  // namespace hiseg

using namespace hiseg;

extern "C" int hiseg_bn_partials(void) { return kBnSplits; }

// Which kernels this thread's last BatchNorm entry point launched (hiseg_bn_last_path, HISEG_BN_PATH_* of
// hiseg_train.h): a host integer written just before the launches; it chooses nothing.
static thread_local int g_bn_last = -1;
extern "C" int hiseg_bn_last_path(void) { return g_bn_last; }

// pixels per iteration of the element-wise BN passes (HISEG_BN_U, read once per call by the plan: A/B timing; the
// same bits, tests/test_gpu_bn_kernels.py).  Two measured no faster (tools/bn_bench.py, profiles/r4_bn_bench.txt:
// apply 5.1-5.4 TB/s, backward 4.3-4.7 TB/s of algorithmic bytes at U = 1 -- 0.7-0.85 of the ~6.3 TB/s a copy
// reaches), so U = 1 stays
static int bn_unroll() {
  const char* e = getenv("HISEG_BN_U");
  return e && atoi(e) == 2 ? 2 : 1;
}

// Pixel splits of the statistics / backward-reduce passes: >= 32 pixels per split, at most kBnSplits (4 blocks per
// CU).  The deep low-resolution layers (the distillation student's 4 x 20 x 20 = 1 600-pixel stages) used to take
// 1 024 one- or two-pixel splits whose merge was most of their BN time.  A function of P alone, so hiseg_bn_stats and
// hiseg_bn_finalize agree.
static int stat_splits(long long P) {
  const long long s = P / 32;
  return (int)(s < 1 ? 1 : s > kBnSplits ? kBnSplits : s);
}
static dim3 fin_grid(int C) { return dim3((unsigned)C); }   // one block per channel

// HISEG_BN_FIN (read per call): 1 bn_finalize_rows_kernel, 0 the per-channel Chan-tree kernel, 2 (default) the rows
// kernel up to 256 splits (a row walks S / 16 of them; more take the per-channel kernel's one round of loads)
static bool bn_fin_rows(int S) {
  const char* e = getenv("HISEG_BN_FIN");
  const int m = e ? atoi(e) : 2;
  return m == 1 || (m == 2 && S <= 256);
}

static void bn_fin_launch(const float* partial, int S, int C, long long P, const float* gamma, const float* beta,
                          float eps, float momentum, float* rm, float* rv, float* mean, float* invstd, float* scale,
                          float* shift, hipStream_t stream, long long rs) {
  const bool rows = bn_fin_rows(S);
  g_bn_last = HISEG_BN_PATH_FINALIZE | (rows ? 0 : HISEG_BN_PATH_PAR);
  if (rows)
    hipLaunchKernelGGL(bn_finalize_rows_kernel, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, stream, partial, S, C,
                       P, gamma, beta, eps, momentum, rm, rv, mean, invstd, scale, shift, rs);
  else
    hipLaunchKernelGGL(bn_finalize_par_kernel, fin_grid(C), dim3(256), 0, stream, partial, S, C, P, gamma, beta, eps,
                       momentum, rm, rv, mean, invstd, scale, shift, rs);
}

extern "C" int hiseg_bn_stats(int dtype, const void* z, long long P, int C, int cstride, int coff, float* partial,
                              hiseg_stream_t stream) {
  HISEG_REQUIRE(z && partial && P > 0 && C > 0 && cstride >= C, HISEG_ERR_BAD_ARG, "bn_stats: bad arguments");
  HISEG_REQUIRE(dtype == HISEG_F32 || dtype == HISEG_BF16, HISEG_ERR_BAD_DTYPE, "bn_stats: dtype");
  const int S = stat_splits(P);   // empty splits write n = 0
  if (vec_ok(dtype, C, z, cstride, coff)) {
    const int V = dtype == HISEG_BF16 ? 8 : 4;
    dim3 grid(S, (C / V + 255) / 256);
    g_bn_last = HISEG_BN_PATH_STATS | HISEG_BN_PATH_VEC;
    DISPATCH_T(dtype, hipLaunchKernelGGL(bn_stats_vec_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, z, P, C,
                                         cstride, coff, partial));
    return hiseg_check_launch("bn_stats");
  }
  dim3 grid(S, (C + 255) / 256);
  g_bn_last = HISEG_BN_PATH_STATS;
  DISPATCH_T(dtype, hipLaunchKernelGGL(bn_stats_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, z, P, C, cstride,
                                       coff, partial));
  return hiseg_check_launch("bn_stats");
}

extern "C" int hiseg_bn_finalize(const float* partial, int C, long long P, const float* gamma, const float* beta,
                                 float eps, float momentum, float* running_mean, float* running_var, float* mean,
                                 float* invstd, float* scale, float* shift, hiseg_stream_t stream) {
  HISEG_REQUIRE(partial && mean && invstd && scale && shift && C > 0, HISEG_ERR_BAD_ARG, "bn_finalize: null");
  bn_fin_launch(partial, stat_splits(P), C, P, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale,
                shift, (hipStream_t)stream, 3ll * C);
  return hiseg_check_launch("bn_finalize");
}

// The same merge over an explicit split count (the fused upsample_bg_fg statistics, ubf_train.hip: 1 024 splits).
int bn_finalize_splits(const float* partial, int S, int C, long long P, const float* gamma, const float* beta,
                       float eps, float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                       float* scale, float* shift, hipStream_t stream, long long rs) {
  bn_fin_launch(partial, S, C, P, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift, stream,
                rs ? rs : 3ll * C);
  return hiseg_check_launch("bn_finalize");
}

extern "C" int hiseg_bn_finalize_n(float* partial, int S, int C, long long P, const float* gamma,
                                   const float* beta, float eps, float momentum, float* running_mean,
                                   float* running_var, float* mean, float* invstd, float* scale, float* shift,
                                   hiseg_stream_t stream) {
  HISEG_REQUIRE(partial && mean && invstd && scale && shift && C > 0 && S > 0 && P > 0, HISEG_ERR_BAD_ARG,
                "bn_finalize_n: bad arguments");
  long long rs = 3ll * C;
  if (S > 4 * KPRE) {   // the conv epilogue's split counts: pre-merged in groups of KPRE first, in place
    const int G = (S + KPRE - 1) / KPRE;
    hipLaunchKernelGGL(bn_premerge_kernel, dim3((C + 63) / 64, G), dim3(256), 0, (hipStream_t)stream, partial, S, C);
    const int e = hiseg_check_launch("bn_premerge");
    if (e) return e;
    S = G;
    rs *= KPRE;
  }
  const int e = bn_finalize_splits(partial, S, C, P, gamma, beta, eps, momentum, running_mean, running_var, mean,
                                   invstd, scale, shift, (hipStream_t)stream, rs);
  if (rs != 3ll * C) g_bn_last |= HISEG_BN_PATH_PREMERGE;
  return e;
}

// One hiseg_bn_bwd call's launch, derived once from the descriptor by bn_bwd_plan: the entry point validates, plans,
// records plan.path and launches.  (hiseg_bn_apply's plan is three locals.)
struct BnPlan {
  bool vec;         // the 16-B chunk kernels (else the scalar ones)
  bool reduce;      // run the reduce pass (else the partials came with the descriptor: partial_splits > 0)
  int mode;         // kGNone .. kGPre
  int unroll;       // HISEG_BN_U, one read
  int S;            // split rows the finalize merges, after any pre-merge; the coefficients follow them
  int G;            // > 0: first sum the partial_splits given rows in G groups of KPRE
  float* partial;   // what finalize and apply read: the descriptor's, or the group region after its rows
  dim3 rgrid, agrid;
  int path;         // what hiseg_bn_last_path reports
};

extern "C" int hiseg_bn_apply(const hiseg_bn_apply_desc* d, hiseg_stream_t stream) {
  HISEG_REQUIRE(d && d->z && d->y && d->scale && d->shift && d->P > 0 && d->C > 0 && d->HW > 0, HISEG_ERR_BAD_ARG,
                "bn_apply: bad arguments");
  HISEG_REQUIRE(d->P < (1ll << 31), HISEG_ERR_BAD_SHAPE, "bn_apply: too many pixels");
  const bool vec = vec_ok(d->dtype, d->C, d->z, d->z_cstride, d->z_coff) &&
                   vec_ok(d->dtype, d->C, d->y, d->y_cstride, d->y_coff) &&
                   vec_ok(d->dtype, d->C, d->residual, d->r_cstride, d->r_coff);
  const int unroll = vec ? bn_unroll() : 1;
  const dim3 grid = vec ? vec_grid(d->P, d->C, d->dtype) : dim3(ew_blocks(d->P * d->C));
  hipStream_t s = (hipStream_t)stream;
  g_bn_last = HISEG_BN_PATH_APPLY | (vec ? HISEG_BN_PATH_VEC : 0) | (unroll == 2 ? HISEG_BN_PATH_U2 : 0);
  if (!vec)
    DISPATCH_T(d->dtype, hipLaunchKernelGGL(bn_apply_kernel<T>, grid, dim3(256), 0, s, *d));
  else if (unroll == 2)
    DISPATCH_T(d->dtype, hipLaunchKernelGGL((bn_apply_vec_kernel<T, 2>), grid, dim3(256), 0, s, *d));
  else
    DISPATCH_T(d->dtype, hipLaunchKernelGGL((bn_apply_vec_kernel<T, 1>), grid, dim3(256), 0, s, *d));
  return hiseg_check_launch("bn_apply");
}

// Group sums of the data-gradient epilogue's backward-reduction partials (hiseg_bn_bwd_desc.partial_splits): block
// (64 channels, KPRE splits), 4 rows x 64 channel lanes, row r summing every 4th split, the rows added in a fixed
// order; group g's sums go to row g of `out` (a region after the partials).
__global__ void __launch_bounds__(256) bn_bwd_premerge_kernel(const float* partial, int S, int C, float* out) {
  __shared__ float a1[4][64], a2[4][64], a3[4][64];
  const int t = threadIdx.x, l = t & 63, r = t >> 6;
  const int c = blockIdx.x * 64 + l;
  const int s0 = blockIdx.y * KPRE;
  float x1 = 0.f, x2 = 0.f, x3 = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int i = r; i < KPRE; i += 4) {
      if (s0 + i >= S) break;
      const float* p = partial + (long long)(s0 + i) * 3 * C;
      x1 += p[c];
      x2 += p[C + c];
      x3 += p[2 * C + c];
    }
  }
  a1[r][l] = x1; a2[r][l] = x2; a3[r][l] = x3;
  __syncthreads();
  if (r == 0 && c < C) {
    float* o = out + (long long)blockIdx.y * 3 * C;
    o[c] = (a1[0][l] + a1[1][l]) + (a1[2][l] + a1[3][l]);
    o[C + c] = (a2[0][l] + a2[1][l]) + (a2[2][l] + a2[3][l]);
    o[2 * C + c] = (a3[0][l] + a3[1][l]) + (a3[2][l] + a3[3][l]);
  }
}

// `partial` holds S rows of [3][C] sums and one row of coefficients after them: S = stat_splits(P) rows of the reduce
// pass, or the partial_splits rows the data-gradient conv's epilogue wrote (hiseg_conv2d_desc.bnb_partial).  More than
// 4 KPRE given rows are first summed into G = ceil(partial_splits / KPRE) group rows after them, and the coefficients
// follow the groups: (partial_splits + G + 1) * 3 * C floats.
static BnPlan bn_bwd_plan(const hiseg_bn_bwd_desc& d) {
  BnPlan pl{};
  const int dt = d.dtype, C = d.C;
  pl.vec = vec_ok(dt, C, d.dy, d.dy_cstride, d.dy_coff) && vec_ok(dt, C, d.y, d.y_cstride, d.y_coff) &&
           vec_ok(dt, C, d.z, d.z_cstride, d.z_coff) && vec_ok(dt, C, d.dz, d.dz_cstride, d.dz_coff) &&
           vec_ok(dt, C, d.dres, d.dres_cstride, d.dres_coff) && vec_ok(dt, C, d.residual, d.r_cstride, d.r_coff);
  pl.reduce = d.partial_splits <= 0;
  pl.mode = bn_bwd_mode(d);
  pl.unroll = pl.vec ? bn_unroll() : 1;
  pl.S = pl.reduce ? stat_splits(d.P) : d.partial_splits;
  pl.partial = d.partial;
  if (!pl.reduce && pl.S > 4 * KPRE) {
    pl.G = (pl.S + KPRE - 1) / KPRE;
    pl.partial += (long long)pl.S * 3 * C;
    pl.S = pl.G;
  }
  pl.rgrid = dim3(pl.S, ((pl.vec ? C / (dt == HISEG_BF16 ? 8 : 4) : C) + 255) / 256);
  pl.agrid = pl.vec ? vec_grid(d.P, C, dt) : dim3(ew_blocks(d.P * C));
  pl.path = HISEG_BN_PATH_BWD | HISEG_BN_PATH_PAR | (pl.mode << HISEG_BN_PATH_MODE_SHIFT) |
            (pl.reduce ? HISEG_BN_PATH_REDUCE : 0) | (pl.G ? HISEG_BN_PATH_PREMERGE : 0) |
            (pl.vec ? HISEG_BN_PATH_VEC : 0) | (pl.unroll == 2 ? HISEG_BN_PATH_U2 : 0);
  return pl;
}

// reduce (unless given), finalize, apply with the chunk kernels of one mode; d.partial is the plan's
template <int MODE>
static void bn_bwd_launch_vec(const BnPlan& pl, const hiseg_bn_bwd_desc& d, hipStream_t s) {
  if (pl.reduce)
    DISPATCH_T(d.dtype, hipLaunchKernelGGL((bn_bwd_reduce_vec_kernel<T, MODE>), pl.rgrid, dim3(256), 0, s, d));
  hipLaunchKernelGGL(bn_bwd_finalize_par_kernel, fin_grid(d.C), dim3(256), 0, s, d, pl.S);
  if (pl.unroll == 2)
    DISPATCH_T(d.dtype, hipLaunchKernelGGL((bn_bwd_apply_vec_kernel<T, MODE, 2>), pl.agrid, dim3(256), 0, s, d, pl.S));
  else
    DISPATCH_T(d.dtype, hipLaunchKernelGGL((bn_bwd_apply_vec_kernel<T, MODE, 1>), pl.agrid, dim3(256), 0, s, d, pl.S));
}

extern "C" int hiseg_bn_bwd(const hiseg_bn_bwd_desc* d_in, hiseg_stream_t stream) {
  HISEG_REQUIRE(d_in, HISEG_ERR_BAD_ARG, "bn_bwd: null descriptor");
  hiseg_bn_bwd_desc d = *d_in;
  HISEG_REQUIRE(d.dy && d.z && d.dz && d.mean && d.invstd && d.partial && d.P > 0 && d.C > 0 && d.HW > 0,
                HISEG_ERR_BAD_ARG, "bn_bwd: bad arguments");
  const bool pre = d.fwd_shift && bn_pre_path(d);
  HISEG_REQUIRE(pre || d.act == HISEG_ACT_NONE || d.act == HISEG_ACT_SILU || d.y, HISEG_ERR_BAD_ARG,
                "bn_bwd: activation needs y");
  HISEG_REQUIRE(pre || (d.act != HISEG_ACT_GELU && d.act != HISEG_ACT_SWISH), HISEG_ERR_BAD_ARG,
                "bn_bwd: GELU / Swish need the forward's fwd_scale / fwd_shift");
  HISEG_REQUIRE(!d.dres || !act_smooth(d.act) || (pre && d.residual), HISEG_ERR_BAD_ARG,
                "bn_bwd: a smooth activation after a residual add needs the residual (pre-activation)");
  HISEG_REQUIRE(d.P < (1ll << 31), HISEG_ERR_BAD_SHAPE, "bn_bwd: too many pixels");
  hipStream_t s = (hipStream_t)stream;
  const BnPlan pl = bn_bwd_plan(d);
  int e = 0;
  if (pl.G) {
    hipLaunchKernelGGL(bn_bwd_premerge_kernel, dim3((d.C + 63) / 64, pl.G), dim3(256), 0, s, d.partial,
                       d.partial_splits, d.C, pl.partial);
    e = hiseg_check_launch("bn_bwd_premerge");
  }
  // a failed pre-merge launch is recorded without the bits of the passes that were not reached
  g_bn_last = e ? pl.path & ~(HISEG_BN_PATH_VEC | HISEG_BN_PATH_U2) : pl.path;
  if (e) return e;
  d.partial = pl.partial;
  if (!pl.vec) {
    if (pl.reduce) DISPATCH_T(d.dtype, hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, pl.rgrid, dim3(256), 0, s, d));
    hipLaunchKernelGGL(bn_bwd_finalize_par_kernel, fin_grid(d.C), dim3(256), 0, s, d, pl.S);
    DISPATCH_T(d.dtype, hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, pl.agrid, dim3(256), 0, s, d, pl.S));
  } else {
    switch (pl.mode) {
      case kGNone: bn_bwd_launch_vec<kGNone>(pl, d, s); break;
      case kGY: bn_bwd_launch_vec<kGY>(pl, d, s); break;
      case kGReLU: bn_bwd_launch_vec<kGReLU>(pl, d, s); break;
      default: bn_bwd_launch_vec<kGPre>(pl, d, s); break;
    }
  }
  return hiseg_check_launch("bn_bwd");
}
