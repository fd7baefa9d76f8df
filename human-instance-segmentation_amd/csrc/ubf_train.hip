#include <cstdlib>
// Training kernels of the refined hierarchical head's last stage (gfx950):
//   * upsample_bg_fg [ConvT 2->32, BatchNorm(train) or LayerNorm2d, act, 1x1 32->2] + softmax + hierarchical
//     combine + the target branch's last 1x1 (refinement.py:501-506,559-596) forward / backward
//   * the target branch's last 1x1 conv (Ct -> 2) backward
//   * sum_rows, the column reducer of these and of spatial attention's weight gradient (declared in train_norm.h)
// All are HBM-streaming kernels; reductions go through deterministic per-block partials and a
// finalize kernel (no atomics).
#include "train_norm.h"
#include "hiseg_head_train.h"

namespace hiseg {

static inline unsigned nb(long long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// out[c] (+)= sum_r part[r*ld + c], c < cols
__global__ void __launch_bounds__(128) sum_rows_kernel(const float* part, int rows, int ld, int cols, float* out, int acc) {
  const int c = blockIdx.x * 128 + threadIdx.x;
  if (c >= cols) return;
  double s = 0;
  for (int r = 0; r < rows; ++r) s += part[(long long)r * ld + c];
  out[c] = acc ? (float)(out[c] + s) : (float)s;
}

// First level of sum_rows for tall inputs: split s (rows [s*R, s*R+R)) of a 64-column tile, 4 row lanes per
// column; the split's sum overwrites its first row (read only by this block), so the second level sums
// ceil(rows/R) rows of stride R*ld.  part is scratch: its contents are consumed.
__global__ void __launch_bounds__(256) sum_rows_split_kernel(float* part, int rows, int ld, int cols, int R) {
  __shared__ double red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), lane = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.y * R;
  const long long r1 = r0 + R < rows ? r0 + R : rows;
  double s = 0;
  if (c < cols)
    for (long long r = r0 + lane; r < r1; r += 4) s += part[r * ld + c];
  red[lane][threadIdx.x & 63] = s;
  __syncthreads();
  if (lane == 0 && c < cols)
    part[r0 * ld + c] = (float)(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

void sum_rows(float* part, int rows, int ld, int cols, float* out, int acc, hipStream_t s) {
  if (rows <= 64) {
    hipLaunchKernelGGL(sum_rows_kernel, dim3((cols + 127) / 128), dim3(128), 0, s, part, rows, ld, cols, out, acc);
    return;
  }
  int R = (rows + 63) / 64;
  R = R < 64 ? 64 : R;
  const int S = (rows + R - 1) / R;
  hipLaunchKernelGGL(sum_rows_split_kernel, dim3((cols + 63) / 64, S), dim3(256), 0, s, part, rows, ld, cols, R);
  hipLaunchKernelGGL(sum_rows_kernel, dim3((cols + 127) / 128), dim3(128), 0, s, part, S, R * ld, cols, out, acc);
}

// ======================================================================================= upsample_bg_fg + combine
struct UbfArgs {
  const float* low; int N, h, w;
  const float* ut_w; const float* ut_b;     // ConvT [2][32][2][2], bias [32]
  const float* scale; const float* shift;   // norm fold: a = act(z*scale + shift); [32] (BN) or [N][32] (LN)
  const float* mean; const float* invstd; const float* gamma;   // [32] (BN) or [N] (LN)
  const float* u1_w; const float* u1_b;     // [2][32], [2]
  int act; float beta; int ln;
};

__device__ __forceinline__ float ubf_z(const UbfArgs& u, float l0, float l1, int c, int q) {
  return l0 * u.ut_w[(c * 2 + (q >> 1)) * 2 + (q & 1)] + l1 * u.ut_w[((32 + c) * 2 + (q >> 1)) * 2 + (q & 1)] + u.ut_b[c];
}

// BN statistics of z = ConvT(low) over all N*2h*2w pixels: partial [S][3][32] (Welford), block = 8 rows x 32 ch
__global__ void __launch_bounds__(256) ubf_stats_kernel(UbfArgs u, float* partial) {
  __shared__ float sn[256], sm[256], sq[256];
  const int t = threadIdx.x, c = t & 31, r = t >> 5;
  const long long P = (long long)u.N * u.h * u.w;
  const long long b = P * blockIdx.x / gridDim.x, e = P * (blockIdx.x + 1) / gridDim.x;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (long long p = b + r; p < e; p += 8) {
    const float l0 = u.low[p * 2], l1 = u.low[p * 2 + 1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float x = ubf_z(u, l0, l1, c, q);
      n += 1.f;
      const float d = x - mean;
      mean += d / n;
      m2 += d * (x - mean);
    }
  }
  sn[t] = n; sm[t] = mean; sq[t] = m2;
  __syncthreads();
  if (r == 0) {
    for (int rr = 1; rr < 8; ++rr) {
      const int o = rr * 32 + c;
      const float nb2 = sn[o];
      if (nb2 == 0.f) continue;
      const float nt = n + nb2, d = sm[o] - mean;
      mean += d * (nb2 / nt);
      m2 += sq[o] + d * d * (n * nb2 / nt);
      n = nt;
    }
    float* out = partial + (long long)blockIdx.x * 96;
    out[c] = n; out[32 + c] = mean; out[64 + c] = m2;
  }
}

// per mask pixel: bg/fg logits, target logits (fused Ct->2 1x1), softmax, hierarchical combine
template <typename T>
__global__ void __launch_bounds__(256) ubf_fwd_kernel(UbfArgs u, const void* tfeat, int Ct, const float* t_w,
                                                      const float* t_b, float* logits, float* bgfg, float* tn) {
  __shared__ float s_tw[2 * 512];
  for (int i = threadIdx.x; i < 2 * Ct; i += 256) s_tw[i] = t_w[i];
  __syncthreads();
  const int H = 2 * u.h, W = 2 * u.w;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)u.N * H * W) return;
  const int X = (int)(gid % W);
  const long long tt = gid / W;
  const int Y = (int)(tt % H);
  const int n = (int)(tt / H);
  const int q = (Y & 1) * 2 + (X & 1);
  const float* lo = u.low + (((long long)n * u.h + (Y >> 1)) * u.w + (X >> 1)) * 2;
  const float l0 = lo[0], l1 = lo[1];
  float b0 = u.u1_b[0], b1 = u.u1_b[1];
  const float* sc = u.scale + (u.ln ? n * 32 : 0);
  const float* sh = u.shift + (u.ln ? n * 32 : 0);
  for (int c = 0; c < 32; ++c) {
    const float a = apply_act(ubf_z(u, l0, l1, c, q) * sc[c] + sh[c], u.act, u.beta);
    b0 += u.u1_w[c] * a;
    b1 += u.u1_w[32 + c] * a;
  }
  constexpr int K = Chunk<T>::N;
  float t0 = t_b[0], t1 = t_b[1], v[K];
  const uint4* tf = reinterpret_cast<const uint4*>(tfeat) + gid * (Ct / K);
  for (int ch = 0; ch < Ct / K; ++ch) {
    Chunk<T>::unpack(tf[ch], v);
#pragma unroll
    for (int e = 0; e < K; ++e) {
      t0 += s_tw[ch * K + e] * v[e];
      t1 += s_tw[Ct + ch * K + e] * v[e];
    }
  }
  const float mx = fmaxf(b0, b1);
  const float e0 = __expf(b0 - mx), e1 = __expf(b1 - mx);
  const float pf = e1 / (e0 + e1);
  const long long plane = (long long)H * W, pp = (long long)Y * W + X;
  float* L = logits + (long long)n * 3 * plane + pp;
  L[0] = b0;
  L[plane] = b1 + t0 * pf;
  L[2 * plane] = b1 + t1 * pf;
  float* G = bgfg + (long long)n * 2 * plane + pp;
  G[0] = b0; G[plane] = b1;
  float* Tn = tn + (long long)n * 2 * plane + pp;
  Tn[0] = t0; Tn[plane] = t1;
}

// pass 1 (8 pixel rows x 32 channels per block): combine backward -> db, dtn per pixel (written by c == 0);
// per channel: sum g, sum g*xhat, sum xhat (BN bwd), dW1[k][c] = sum db_k * a_c; db1.
// partial layout per block: [32 g][32 gx][32 x][64 dW1][2 db1]  (162)
// LayerNorm (u.ln): sb blocks per sample, block j of sample n covers a slice of that sample only, so the
// per-block channel sums add up to per-(sample, channel) sums.
template <bool U2>
__global__ void __launch_bounds__(256) ubf_bwd1_kernel(UbfArgs u, const float* dlogits, const float* dbgfg_ext,
                                                       const float* dtn_ext, const float* bgfg, const float* tn,
                                                       float* db_out, float* dtn_out, float* partial, int sb) {
  __shared__ float red[8][162];
  const int t = threadIdx.x, c = t & 31, r = t >> 5;
  const int H = 2 * u.h, W = 2 * u.w;
  const long long P = (long long)u.N * H * W, plane = (long long)H * W;
  long long b, e;
  int ns = 0;
  if (u.ln) {
    ns = blockIdx.x / sb;
    const int j = blockIdx.x % sb;
    b = ns * plane + plane * j / sb;
    e = ns * plane + plane * (j + 1) / sb;
  } else {
    b = P * blockIdx.x / gridDim.x;
    e = P * (blockIdx.x + 1) / gridDim.x;
  }
  const float mu = u.ln ? u.mean[ns] : u.mean[c], inv = u.ln ? u.invstd[ns] : u.invstd[c];
  const float scc = u.ln ? u.scale[ns * 32 + c] : u.scale[c], shc = u.ln ? u.shift[ns * 32 + c] : u.shift[c];
  const float w0 = u.u1_w[c], w1 = u.u1_w[32 + c];
  // the thread's ConvTranspose weights for the 4 sub-pixels and its bias, loaded once (U2; the U1 form re-reads them
  // per pixel through ubf_z: the stores below may alias them as far as the compiler knows)
  float zw0[4], zw1[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    zw0[q] = u.ut_w[(c * 2 + (q >> 1)) * 2 + (q & 1)];
    zw1[q] = u.ut_w[((32 + c) * 2 + (q >> 1)) * 2 + (q & 1)];
  }
  const float zb = u.ut_b[c];
  float sg = 0.f, sgx = 0.f, sx = 0.f, dw0 = 0.f, dw1 = 0.f, db0s = 0.f, db1s = 0.f;
  // (n, Y, X) of p advanced incrementally by the row stride 8: the 64-bit div / mod per pixel dominated the loop
  int X, Y;
  long long n;
  {
    const long long p0 = b + r, tt = p0 / W;
    X = (int)(p0 - tt * W);
    Y = (int)(tt % H);
    n = tt / H;
  }
  struct In { float g0, g1, t0, t1, dL0, dL1, dL2, e0, e1, f0, f1, l0, l1; long long pp, n; int X, Y; };
  auto load = [&](long long nn, int YY, int XX) __attribute__((always_inline)) -> In {
    In v;
    const long long pp = (long long)YY * W + XX;
    const float* G = bgfg + nn * 2 * plane + pp;
    const float* Tn = tn + nn * 2 * plane + pp;
    const float* dL = dlogits + nn * 3 * plane + pp;
    v.g0 = G[0]; v.g1 = G[plane]; v.t0 = Tn[0]; v.t1 = Tn[plane];
    v.dL0 = dL[0]; v.dL1 = dL[plane]; v.dL2 = dL[2 * plane];
    v.e0 = dbgfg_ext ? dbgfg_ext[nn * 2 * plane + pp] : 0.f;
    v.e1 = dbgfg_ext ? dbgfg_ext[nn * 2 * plane + plane + pp] : 0.f;
    v.f0 = dtn_ext ? dtn_ext[nn * 2 * plane + pp] : 0.f;
    v.f1 = dtn_ext ? dtn_ext[nn * 2 * plane + plane + pp] : 0.f;
    const float* lo = u.low + ((nn * u.h + (YY >> 1)) * u.w + (XX >> 1)) * 2;
    v.l0 = lo[0]; v.l1 = lo[1];
    v.pp = pp; v.n = nn; v.X = XX; v.Y = YY;
    return v;
  };
  auto body = [&](const In& v, long long p) __attribute__((always_inline)) {
    const float mx = fmaxf(v.g0, v.g1);
    const float ex0 = __expf(v.g0 - mx), ex1 = __expf(v.g1 - mx);
    const float pf = ex1 / (ex0 + ex1);
    const float dpf = v.dL1 * v.t0 + v.dL2 * v.t1;
    const float dsg = dpf * pf * (1.f - pf);
    float db0 = v.dL0 - dsg, db1 = v.dL1 + v.dL2 + dsg;
    float dt0 = v.dL1 * pf, dt1 = v.dL2 * pf;
    if (dbgfg_ext) { db0 += v.e0; db1 += v.e1; }
    if (dtn_ext) { dt0 += v.f0; dt1 += v.f1; }
    if (c == 0) {
      db_out[p * 2] = db0; db_out[p * 2 + 1] = db1;
      dtn_out[p * 2] = dt0; dtn_out[p * 2 + 1] = dt1;
      db0s += db0; db1s += db1;
    }
    const int q = (v.Y & 1) * 2 + (v.X & 1);
    const float z = U2 ? v.l0 * zw0[q] + v.l1 * zw1[q] + zb : ubf_z(u, v.l0, v.l1, c, q);
    const float pre = z * scc + shc;
    const float a = apply_act(pre, u.act, u.beta);
    const float g = (w0 * db0 + w1 * db1) * act_grad_pre(pre, u.act, u.beta);
    const float xh = (z - mu) * inv;
    sg += g; sgx += g * xh; sx += xh;
    dw0 += db0 * a; dw1 += db1 * a;
  };
  auto step = [&]() __attribute__((always_inline)) {
    X += 8;
    while (X >= W) {
      X -= W;
      if (++Y == H) { Y = 0; ++n; }
    }
  };
  long long p = b + r;
  while (X >= W) {   // (b + r may start past a row end only through the initial decomposition: never; kept for form)
    X -= W;
    if (++Y == H) { Y = 0; ++n; }
  }
  if (U2) {
    // two pixels per iteration, both pixels' loads issued before either's arithmetic; the sums in pixel order
    for (; p + 8 < e; p += 16) {
      const In va = load(n, Y, X);
      step();
      const In vb = load(n, Y, X);
      step();
      body(va, p);
      body(vb, p + 8);
    }
  }
  for (; p < e; p += 8) {
    const In va = load(n, Y, X);
    step();
    body(va, p);
  }
  red[r][c] = sg; red[r][32 + c] = sgx; red[r][64 + c] = sx; red[r][96 + c] = dw0; red[r][128 + c] = dw1;
  if (c == 0) { red[r][160] = db0s; red[r][161] = db1s; }
  __syncthreads();
  if (t < 162) {
    float s = 0.f;
    for (int rr = 0; rr < 8; ++rr) s += red[rr][t];
    partial[(long long)blockIdx.x * 162 + t] = s;
  }
}

// finalize 1: BN coefficients + dgamma/dbeta/dW1/db1 (accumulate into the parameter gradients)
// coef: [32 k][32 mean g][32 mean gx]
__global__ void ubf_fin1_kernel(UbfArgs u, const float* partial, int nblk, long long P, float* coef, float* dgamma,
                                float* dbeta, float* du1_w, float* du1_b, float* dut_b_analytic) {
  const int t = threadIdx.x;
  if (t >= 162) return;
  // 8 independent partial sums, 16 loads in flight per thread: the serial dependent loop over 2048 block rows
  // was latency-bound (0.5 ms for one 192-thread block)
  double s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int b = 0;
  for (; b + 16 <= nblk; b += 16) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = partial[(long long)(b + i) * 162 + t];
#pragma unroll
    for (int i = 0; i < 16; ++i) s8[i & 7] += v[i];
  }
  for (; b < nblk; ++b) s8[0] += partial[(long long)b * 162 + t];
  const double s = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
  __shared__ double S[162];
  S[t] = s;
  __syncthreads();
  if (t < 32) {
    const double k = u.ln ? 0.0 : (u.gamma ? u.gamma[t] : 1.0) * u.invstd[t];   // BN coefficients only
    coef[t] = (float)k;
    coef[32 + t] = (float)(S[t] / P);
    coef[64 + t] = (float)(S[32 + t] / P);
    dgamma[t] += (float)S[32 + t];
    dbeta[t] += (float)S[t];
    if (dut_b_analytic) dut_b_analytic[t] += (float)(k * (S[t] - P * (S[t] / P) - S[64 + t] * (S[32 + t] / P)));
  }
  if (t >= 96 && t < 160) du1_w[t - 96] += (float)S[t];
  if (t >= 160) du1_b[t - 160] += (float)S[t];
}

// LayerNorm finalize (grid N, 32 lanes): the sample's sb block partials -> G, GX, X per channel,
// coef_ln[n] = (a_n, b_n), dbias[n][c] = invstd_n (gamma_c G - HWm a_n - X b_n) (the ConvTranspose bias gradient)
__global__ void ubf_ln_fin_kernel(UbfArgs u, const float* partial, int sb, float* coef_ln, float* dbias) {
  __shared__ float sa[32], sbb[32];
  const int n = blockIdx.x, c = threadIdx.x;
  double G = 0, GX = 0, X = 0;
  for (int j = 0; j < sb; ++j) {
    const float* q = partial + ((long long)n * sb + j) * 162;
    G += q[c]; GX += q[32 + c]; X += q[64 + c];
  }
  const float gam = u.gamma ? u.gamma[c] : 1.f;
  sa[c] = (float)(gam * G); sbb[c] = (float)(gam * GX);
  __syncthreads();
  double A = 0, B = 0;
  for (int i = 0; i < 32; ++i) { A += sa[i]; B += sbb[i]; }
  const double HWm = 4.0 * u.h * u.w, M = 32.0 * HWm;
  const double an = A / M, bn = B / M;
  if (c == 0) { coef_ln[n * 2] = (float)an; coef_ln[n * 2 + 1] = (float)bn; }
  dbias[n * 32 + c] = (float)(u.invstd[n] * (gam * G - HWm * an - X * bn));
}

// pass 2 (per low pixel, 8 rows x 32 channels): dz of the 4 children, dlow, dWt partial [ci][c][q] (256)
// LayerNorm: coef_ln [N][2] = (a_n, b_n); dz = invstd_n * (gamma_c g - a_n - xhat b_n)
__global__ void __launch_bounds__(256) ubf_bwd2_kernel(UbfArgs u, const float* db_in, const float* coef,
                                                       const float* coef_ln, float* dlow, float* partial) {
  __shared__ float red[8][256];
  const int t = threadIdx.x, c = t & 31, r = t >> 5;
  const long long PL = (long long)u.N * u.h * u.w;
  const long long b = PL * blockIdx.x / gridDim.x, e = PL * (blockIdx.x + 1) / gridDim.x;
  const float k = u.ln ? 0.f : coef[c], m1 = u.ln ? 0.f : coef[32 + c], m2 = u.ln ? 0.f : coef[64 + c];
  const float gam = u.gamma ? u.gamma[c] : 1.f;
  const float w0 = u.u1_w[c], w1 = u.u1_w[32 + c];
  const int W = 2 * u.w;
  float dw[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) dw[i] = 0.f;
  int x, y;
  long long n;
  {
    const long long p0 = b + r, tt = p0 / u.w;
    x = (int)(p0 - tt * u.w);
    y = (int)(tt % u.h);
    n = tt / u.h;
  }
  for (long long p = b + r; p < e; p += 8, x += 8) {
    while (x >= u.w) {
      x -= u.w;
      if (++y == u.h) { y = 0; ++n; }
    }
    const float l0 = u.low[p * 2], l1 = u.low[p * 2 + 1];
    const float mu = u.ln ? u.mean[n] : u.mean[c], inv = u.ln ? u.invstd[n] : u.invstd[c];
    const float scc = u.ln ? u.scale[n * 32 + c] : u.scale[c], shc = u.ln ? u.shift[n * 32 + c] : u.shift[c];
    float dl0 = 0.f, dl1 = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long P = (n * (2 * u.h) + 2 * y + (q >> 1)) * W + 2 * x + (q & 1);
      const float z = ubf_z(u, l0, l1, c, q);
      const float pre = z * scc + shc;
      const float g = (w0 * db_in[P * 2] + w1 * db_in[P * 2 + 1]) * act_grad_pre(pre, u.act, u.beta);
      const float dz = u.ln ? inv * (gam * g - coef_ln[n * 2] - (z - mu) * inv * coef_ln[n * 2 + 1])
                            : k * (g - m1 - (z - mu) * inv * m2);
      const float wa = u.ut_w[(c * 2 + (q >> 1)) * 2 + (q & 1)];
      const float wb = u.ut_w[((32 + c) * 2 + (q >> 1)) * 2 + (q & 1)];
      dl0 += wa * dz;
      dl1 += wb * dz;
      dw[q] += l0 * dz;
      dw[4 + q] += l1 * dz;
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      dl0 += __shfl_xor(dl0, off, 32);
      dl1 += __shfl_xor(dl1, off, 32);
    }
    if (c == 0) { dlow[p * 2] = dl0; dlow[p * 2 + 1] = dl1; }
  }
  // layout [ci][c][q] -> index (ci*32 + c)*4 + q
#pragma unroll
  for (int q = 0; q < 4; ++q) { red[r][(0 * 32 + c) * 4 + q] = dw[q]; red[r][(1 * 32 + c) * 4 + q] = dw[4 + q]; }
  __syncthreads();
  float s = 0.f;
  for (int rr = 0; rr < 8; ++rr) s += red[rr][t];
  partial[(long long)blockIdx.x * 256 + t] = s;
}

// ======================================================================================= last 1x1 (Ct -> 2) backward
// dt[p][c] = sum_k dtn[p][k] * w[k][c]; dW[k][c] = sum_p dtn[p][k] * t[p][c]; db[k] = sum_p dtn[p][k]
// block: 16 pixel rows x (Ct/K) chunk lanes
template <typename T>
__global__ void __launch_bounds__(256) pw2_bwd_kernel(const void* tfeat, long long P, int Ct, const float* dtn,
                                                      const float* w, void* dt, float* partial) {
  constexpr int K = Chunk<T>::N;
  extern __shared__ float red[];  // [R][2*Ct + 2]
  const int nch = Ct / K;
  const int R = 256 / nch;
  const int t = threadIdx.x, ch = t % nch, r = t / nch;
  const long long b = P * blockIdx.x / gridDim.x, e = P * (blockIdx.x + 1) / gridDim.x;
  float a0[K], a1[K], v[K], wk0[K], wk1[K];
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) { a0[i] = 0.f; a1[i] = 0.f; wk0[i] = w[ch * K + i]; wk1[i] = w[Ct + ch * K + i]; }
  if (r < R) {
    for (long long p = b + r; p < e; p += R) {
      const float d0 = dtn[p * 2], d1 = dtn[p * 2 + 1];
      Chunk<T>::unpack(reinterpret_cast<const uint4*>(tfeat)[p * nch + ch], v);
      float o[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        a0[i] += d0 * v[i];
        a1[i] += d1 * v[i];
        o[i] = d0 * wk0[i] + d1 * wk1[i];
      }
      reinterpret_cast<uint4*>(dt)[p * nch + ch] = Chunk<T>::pack(o);
      if (ch == 0) { s0 += d0; s1 += d1; }
    }
  }
  const int cols = 2 * Ct + 2;
  if (r < R) {
#pragma unroll
    for (int i = 0; i < K; ++i) { red[r * cols + ch * K + i] = a0[i]; red[r * cols + Ct + ch * K + i] = a1[i]; }
    if (ch == 0) { red[r * cols + 2 * Ct] = s0; red[r * cols + 2 * Ct + 1] = s1; }
  }
  __syncthreads();
  for (int i = t; i < cols; i += 256) {
    float s = 0.f;
    for (int rr = 0; rr < R; ++rr) s += red[rr * cols + i];
    partial[(long long)blockIdx.x * cols + i] = s;
  }
}

}  // namespace hiseg

using namespace hiseg;

static UbfArgs ubf_args(const hiseg_ubf_desc* d) {
  UbfArgs u;
  u.low = d->low; u.N = d->N; u.h = d->h; u.w = d->w;
  u.ut_w = d->ut_w; u.ut_b = d->ut_b;
  u.scale = d->scale; u.shift = d->shift; u.mean = d->mean; u.invstd = d->invstd; u.gamma = d->gamma;
  u.u1_w = d->u1_w; u.u1_b = d->u1_b;
  u.act = d->act; u.beta = d->act_beta; u.ln = d->layernorm;
  return u;
}

// blocks of the pass-1 reduction: kUbfBlocks pixel ranges (BN), or sb ranges per sample (LN)
static int ubf_sb(int N) { const int sb = 2048 / (N > 0 ? N : 1); return sb < 1 ? 1 : sb; }

static const int kUbfBlocks = 2048;   // 8 workgroups per CU: the per-pixel loops are latency-bound

// The backward's workspace, as float offsets into ws: the block partials at 0 -- pass 1's [nb1][162] (nb1 = N sb under
// LayerNorm, at most kUbfBlocks otherwise), then pass 2's [kUbfBlocks][256], so the larger of the two -- followed by
// coef [96] (BN), coef_ln [N][2] and dbias [N][32] (LN).
struct UbfWs { long long coef, coef_ln, dbias, total; };

static UbfWs ubf_ws_layout(int N) {
  const long long p1 = (long long)N * ubf_sb(N) * 162, p2 = (long long)kUbfBlocks * 256;
  UbfWs l;
  l.coef = p1 > p2 ? p1 : p2;
  l.coef_ln = l.coef + 96;
  l.dbias = l.coef_ln + 2LL * N;
  l.total = l.dbias + 32LL * N;
  return l;
}

extern "C" int hiseg_ubf_ws(int N) {
  const long long bwd = ubf_ws_layout(N).total;
  const long long fwd = (long long)hiseg_bn_partials() * 96;
  return (int)(bwd > fwd ? bwd : fwd);
}

extern "C" int hiseg_ubf_train_fwd(const hiseg_ubf_desc* d, float eps, float momentum, float* running_mean,
                                   float* running_var, float* ws, hiseg_stream_t stream) {
  HISEG_REQUIRE(d && d->low && d->ut_w && d->ut_b && d->u1_w && d->u1_b && d->tfeat && d->t_w && d->t_b && d->logits &&
                    d->bgfg && d->tn && ws && d->scale && d->shift && d->mean && d->invstd,
                HISEG_ERR_BAD_ARG, "ubf_train_fwd: null argument");
  HISEG_REQUIRE(d->Ct > 0 && d->Ct <= 512 && d->Ct % chunk_of(d->dtype) == 0, HISEG_ERR_BAD_SHAPE, "ubf: Ct");
  HISEG_REQUIRE(d->act >= HISEG_ACT_NONE && d->act <= HISEG_ACT_SWISH, HISEG_ERR_BAD_ARG, "ubf: activation");
  hipStream_t s = (hipStream_t)stream;
  const UbfArgs u = ubf_args(d);
  const long long Pm = (long long)d->N * 4 * d->h * d->w;
  if (d->layernorm) {   // per-sample statistics; no running statistics
    int r = hiseg_ubf_ln_tables(d->low, d->N, d->h, d->w, d->ut_w, d->ut_b, d->gamma, d->beta, eps, 0,
                                const_cast<float*>(d->mean), const_cast<float*>(d->invstd), const_cast<float*>(d->scale),
                                const_cast<float*>(d->shift), stream);
    if (r) return r;
  } else {
    const int S = hiseg_bn_partials();
    hipLaunchKernelGGL(ubf_stats_kernel, dim3(S), dim3(256), 0, s, u, ws);
    int r = bn_finalize_splits(ws, S, 32, Pm, d->gamma, d->beta, eps, momentum, running_mean, running_var,
                               const_cast<float*>(d->mean), const_cast<float*>(d->invstd), const_cast<float*>(d->scale),
                               const_cast<float*>(d->shift), s);
    if (r) return r;
  }
  DISPATCH_T(d->dtype, hipLaunchKernelGGL(ubf_fwd_kernel<T>, dim3(nb(Pm, 256)), dim3(256), 0, s, u, d->tfeat, d->Ct,
                                          d->t_w, d->t_b, d->logits, d->bgfg, d->tn));
  return hiseg_check_launch("ubf_train_fwd");
}

extern "C" int hiseg_ubf_train_bwd(const hiseg_ubf_desc* d, const float* dlogits, const float* dbgfg_ext,
                                   const float* dtn_ext, float* db_buf, float* dtn_out, float* dlow, float* ws,
                                   const hiseg_ubf_grads* g, hiseg_stream_t stream) {
  HISEG_REQUIRE(d && dlogits && db_buf && dtn_out && dlow && ws && g && g->dut_w && g->dut_b && g->dgamma && g->dbeta &&
                    g->du1_w && g->du1_b,
                HISEG_ERR_BAD_ARG, "ubf_train_bwd: null argument");
  hipStream_t s = (hipStream_t)stream;
  const UbfArgs u = ubf_args(d);
  const long long Pm = (long long)d->N * 4 * d->h * d->w;
  const int sb = ubf_sb(d->N);
  const int nb1 = d->layernorm ? d->N * sb : kUbfBlocks;
  const UbfWs l = ubf_ws_layout(d->N);
  float* part = ws;   // [nb1][162] (pass 1), then [kUbfBlocks][256] (pass 2)
  float* coef = ws + l.coef;
  float* coef_ln = ws + l.coef_ln;
  float* dbias = ws + l.dbias;
  // HISEG_UBF_U2=0: the one-pixel loop with per-pixel weight reads (A/B timing; same results)
  const char* ue = getenv("HISEG_UBF_U2");
  if (!(ue && atoi(ue) == 0))
    hipLaunchKernelGGL(ubf_bwd1_kernel<true>, dim3(nb1), dim3(256), 0, s, u, dlogits, dbgfg_ext, dtn_ext, d->bgfg,
                       d->tn, db_buf, dtn_out, part, sb);
  else
    hipLaunchKernelGGL(ubf_bwd1_kernel<false>, dim3(nb1), dim3(256), 0, s, u, dlogits, dbgfg_ext, dtn_ext, d->bgfg,
                       d->tn, db_buf, dtn_out, part, sb);
  if (d->layernorm)
    hipLaunchKernelGGL(ubf_ln_fin_kernel, dim3(d->N), dim3(32), 0, s, u, part, sb, coef_ln, dbias);
  hipLaunchKernelGGL(ubf_fin1_kernel, dim3(1), dim3(192), 0, s, u, part, nb1, Pm, coef, g->dgamma, g->dbeta,
                     g->du1_w, g->du1_b, d->layernorm ? nullptr : g->dut_b);
  if (d->layernorm) sum_rows(dbias, d->N, 32, 32, g->dut_b, 1, s);
  hipLaunchKernelGGL(ubf_bwd2_kernel, dim3(kUbfBlocks), dim3(256), 0, s, u, db_buf, coef, coef_ln, dlow, part);
  // dWt [ci][c][q] in the ConvTranspose2d layout [2][32][2][2] == (ci*32 + c)*4 + q
  sum_rows(part, kUbfBlocks, 256, 256, g->dut_w, 1, s);
  return hiseg_check_launch("ubf_train_bwd");
}

static const int kPw2Blocks = 512;
extern "C" int hiseg_pw2_ws(int Ct) { return kPw2Blocks * (2 * Ct + 2); }

extern "C" int hiseg_pw2_bwd(int dtype, const void* tfeat, long long P, int Ct, const float* dtn, const float* w,
                             void* dt, float* ws, float* dw, float* db, hiseg_stream_t stream) {
  HISEG_REQUIRE(tfeat && dtn && w && dt && ws && dw && db && P > 0, HISEG_ERR_BAD_ARG, "pw2_bwd: null argument");
  HISEG_REQUIRE(Ct % chunk_of(dtype) == 0 && Ct / chunk_of(dtype) <= 256, HISEG_ERR_BAD_SHAPE, "pw2_bwd: Ct");
  hipStream_t s = (hipStream_t)stream;
  const int nch = Ct / chunk_of(dtype);
  const int R = 256 / nch;
  const size_t lds = (size_t)R * (2 * Ct + 2) * sizeof(float);
  DISPATCH_T(dtype, hipLaunchKernelGGL(pw2_bwd_kernel<T>, dim3(kPw2Blocks), dim3(256), lds, s, tfeat, P, Ct, dtn, w, dt, ws));
  sum_rows(ws, kPw2Blocks, 2 * Ct + 2, 2 * Ct, dw, 1, s);
  sum_rows(ws + 2 * Ct, kPw2Blocks, 2 * Ct + 2, 2, db, 1, s);
  return hiseg_check_launch("pw2_bwd");
}
