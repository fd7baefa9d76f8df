// The device code of PretrainedUNetGuidedSegmentationHead that the conv kernels cannot express
// (include/hiseg_guided_head.h).
//
//   guided_prep        : per pixel p = sigmoid(m) -> the compute-dtype chunk input_adjust's loader reads as source B
//                        (+ optional f32 p and the guidance factor 0.5 + 0.5 p)
//   guided_attn        : per pixel sigmoid(w2 . act(W1 y + b1) + b2) * factor; one thread per pixel with the 64 hidden
//                        accumulators in registers and W1 read through wave-uniform (scalar) loads -- any dtype
//   guided_attn_mfma   : the same for bf16 y with 256 channels on mfma_f32_16x16x32_bf16: W1 is the A operand (held in
//                        registers for the kernel's lifetime), 16 pixels are the B operand straight from global memory
//                        (a lane's 8 channels are one 16-byte chunk of the channel-last pixel), the 64 -> 1 dot product
//                        runs on the accumulators and two cross-lane adds
//   guided_finish      : a workgroup owns a run of output rows of one ROI: the 1x1 C -> 3 over the source rows they
//                        need goes to LDS (16 lanes per pixel, one 16-byte chunk per lane and step), then each thread
//                        resizes the three logits and the mask logit for its output pixels and writes logits and aux
//
// The sigmoid of the mask logit and the two logs are plain IEEE f32 (expf, a correctly rounded division, logf): where
// the probability saturates, log(1 - p + 1e-7) depends on the last bit of p, so the fast reciprocal is not used here.
#include "common.h"
#include "gfx950_prims.h"
#include "hiseg_guided_head.h"

#include <math.h>

namespace {

using namespace hiseg;

constexpr int kT = 256;         // threads per block
constexpr int kHidden = 64;     // attention hidden width (mid_channels / 4 of the 256-channel head)
constexpr int kFinishLds = 48 * 1024;

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ float sigmoid_ieee(float v) { return 1.0f / (1.0f + expf(-v)); }

// ------------------------------------------------------------------ guidance prep
template <typename T>
__global__ void __launch_bounds__(kT) guided_prep_kernel(hiseg_guided_prep_desc d) {
  const long long plane = (long long)d.h * d.w;
  const long long q = (long long)blockIdx.x * kT + threadIdx.x;
  if (q >= (long long)d.N * plane) return;
  const long long n = q / plane, r = q % plane;
  const float p = sigmoid_ieee(d.mask[n * d.mask_stride + r]);
  // one 16-byte chunk: p in element 0, the pad channels zero
  const unsigned first = std::is_same<T, float>::value ? __float_as_uint(p) : (unsigned)f2bf(p);
  char* dst = reinterpret_cast<char*>(d.fgp_c) + (q * d.fgp_cstride + d.fgp_coff) * (long long)(16 / Chunk<T>::N);
  *reinterpret_cast<uint4*>(dst) = make_uint4(first, 0u, 0u, 0u);
  if (d.fg_prob) d.fg_prob[q] = p;
  if (d.factor) d.factor[q] = 0.5f + 0.5f * p;
}

// ------------------------------------------------------------------ attention gate
template <typename T>
__global__ void __launch_bounds__(kT) guided_attn_kernel(hiseg_guided_attn_desc d) {
  constexpr int K = Chunk<T>::N;
  const long long p = (long long)blockIdx.x * kT + threadIdx.x;
  if (p >= d.P) return;
  const int nch = d.C / K;
  const float* __restrict__ w1t = d.w1t;
  float acc[kHidden];
#pragma unroll
  for (int j = 0; j < kHidden; ++j) acc[j] = d.b1[j];
  const uint4* src = reinterpret_cast<const uint4*>(d.x) + p * nch;
  for (int ch = 0; ch < nch; ++ch) {
    float v[K];
    Chunk<T>::unpack(src[ch], v);
#pragma unroll
    for (int e = 0; e < K; ++e) {
      const float* wr = w1t + (long long)(ch * K + e) * kHidden;   // wave-uniform address
#pragma unroll
      for (int j = 0; j < kHidden; ++j) acc[j] = fmaf(v[e], wr[j], acc[j]);
    }
  }
  float s = d.b2[0];
#pragma unroll
  for (int j = 0; j < kHidden; ++j) s = fmaf(d.w2[j], apply_act(acc[j], d.act, d.act_beta), s);
  const float a = sigmoid_ieee(s);
  if (d.att) d.att[p] = a;
  d.gate[p] = a * d.factor[p];
}

// bf16, C = 256: 8 k-steps of 32 channels, 4 row tiles of 16 hidden units.  One wave per SIMD (the 32 A fragments
// take 128 registers); a wave walks 16-pixel groups.
__global__ void __launch_bounds__(kT) guided_attn_mfma_kernel(hiseg_guided_attn_desc d) {
  constexpr int KS = 8, MT = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lg = lane >> 4, col = lane & 15;
  const uint4* wf = reinterpret_cast<const uint4*>(d.w1_frag);
  uint4 af[MT][KS];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int s = 0; s < KS; ++s) af[t][s] = wf[(t * KS + s) * 64 + lane];
  float bb[MT][4], ww[MT][4];   // the accumulator's rows: hidden unit 16 t + 4 lg + i
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bb[t][i] = d.b1[16 * t + 4 * lg + i];
      ww[t][i] = d.w2[16 * t + 4 * lg + i];
    }
  const float b2 = d.b2[0];
  const long long groups = (d.P + 15) / 16;
  for (long long g = (long long)blockIdx.x * 4 + wave; g < groups; g += (long long)gridDim.x * 4) {
    const long long pix = g * 16 + col;
    const long long pc = pix < d.P ? pix : d.P - 1;   // lanes past the end read the last pixel and write nothing
    const uint4* src = reinterpret_cast<const uint4*>(d.x) + pc * (4 * KS) + lg;
    uint4 bf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) bf[s] = src[4 * s];
    floatx4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[t][s]),
                                                         __builtin_bit_cast(bf16x8_t, bf[s]), acc[t], 0, 0, 0);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) sum = fmaf(ww[t][i], apply_act(acc[t][i] + bb[t][i], d.act, d.act_beta), sum);
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (lg == 0 && pix < d.P) {
      const float a = sigmoid_ieee(sum + b2);
      if (d.att) d.att[pix] = a;
      d.gate[pix] = a * d.factor[pix];
    }
  }
}

// ------------------------------------------------------------------ finish
// Source coordinate of output index o (F.interpolate, bilinear, align_corners = False): the lower tap, the upper tap
// and the upper tap's weight.
__device__ __forceinline__ void src_taps(int o, float scale, int n_in, int& i0, int& i1, float& l) {
  float s = ((float)o + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l = s - (float)i0;
}

__device__ __forceinline__ float lerp2(float a, float b, float c, float e, float ly, float lx) {
  return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * e);
}

template <typename T>
__global__ void __launch_bounds__(kT) guided_finish_kernel(hiseg_guided_finish_desc d, int rows, int cap_rows, int tiles) {
  constexpr int K = Chunk<T>::N;
  constexpr int G = 16;
  extern __shared__ float lds[];   // [3][cap_rows * w]
  const long long n = blockIdx.x / tiles;
  const int o0 = (int)(blockIdx.x % tiles) * rows;
  const int o1 = o0 + rows < d.mh ? o0 + rows : d.mh;
  const bool same = d.mh == d.h && d.mw == d.w;
  const float sh = (float)d.h / (float)d.mh, sw = (float)d.w / (float)d.mw;
  int s0, s1;
  if (same) {
    s0 = o0;
    s1 = o1 - 1;
  } else {
    int t;
    float l;
    src_taps(o0, sh, d.h, s0, t, l);
    src_taps(o1 - 1, sh, d.h, t, s1, l);
  }
  if (s1 - s0 + 1 > cap_rows) s1 = s0 + cap_rows - 1;   // (never: the host sized cap_rows with slack)
  const int srows = s1 - s0 + 1;
  const int cap = cap_rows * d.w;
  const int npx = srows * d.w;
  const int nch = d.C / K;
  const int l16 = threadIdx.x & (G - 1), sub = threadIdx.x / G;
  const uint4* zrow = reinterpret_cast<const uint4*>(d.z) + ((n * d.h + s0) * (long long)d.w) * nch;
  for (int base = 0; base < npx; base += kT / G) {
    const int q = base + sub;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (q < npx) {
      const uint4* src = zrow + (long long)q * nch;
      for (int ch = l16; ch < nch; ch += G) {
        float v[K];
        Chunk<T>::unpack(src[ch], v);
#pragma unroll
        for (int e = 0; e < K; ++e) {
          const int c = ch * K + e;
          a0 = fmaf(v[e], d.w3[c], a0);
          a1 = fmaf(v[e], d.w3[d.C + c], a1);
          a2 = fmaf(v[e], d.w3[2 * d.C + c], a2);
        }
      }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      a0 += __shfl_xor(a0, off, G);
      a1 += __shfl_xor(a1, off, G);
      a2 += __shfl_xor(a2, off, G);
    }
    if (q < npx && l16 == 0) {
      lds[q] = a0 + d.b3[0];
      lds[cap + q] = a1 + d.b3[1];
      lds[2 * cap + q] = a2 + d.b3[2];
    }
  }
  __syncthreads();
  const long long oplane = (long long)d.mh * d.mw;
  const bool aux = d.bg_fg_logits || d.fg_prob || d.mask_out;
  const float* mk = d.mask ? d.mask + n * d.mask_stride : nullptr;
  const int nout = (o1 - o0) * d.mw;
  for (int idx = threadIdx.x; idx < nout; idx += kT) {
    const int oy = o0 + idx / d.mw, ox = idx % d.mw;
    float v0, v1, v2, m = 0.f;
    if (same) {
      int r = oy - s0;
      r = r < srows ? r : srows - 1;
      const int at = r * d.w + ox;
      v0 = lds[at];
      v1 = lds[cap + at];
      v2 = lds[2 * cap + at];
      if (aux) m = mk[oy * d.w + ox];
    } else {
      int y0, y1, x0, x1;
      float ly, lx;
      src_taps(oy, sh, d.h, y0, y1, ly);
      src_taps(ox, sw, d.w, x0, x1, lx);
      if (aux) m = lerp2(mk[y0 * d.w + x0], mk[y0 * d.w + x1], mk[y1 * d.w + x0], mk[y1 * d.w + x1], ly, lx);
      int r0 = y0 - s0, r1 = y1 - s0;   // inside [0, srows) by the monotonicity of src_taps; clamped all the same
      r0 = r0 < 0 ? 0 : (r0 < srows ? r0 : srows - 1);
      r1 = r1 < 0 ? 0 : (r1 < srows ? r1 : srows - 1);
      const int a = r0 * d.w + x0, b = r0 * d.w + x1, c = r1 * d.w + x0, e = r1 * d.w + x1;
      v0 = lerp2(lds[a], lds[b], lds[c], lds[e], ly, lx);
      v1 = lerp2(lds[cap + a], lds[cap + b], lds[cap + c], lds[cap + e], ly, lx);
      v2 = lerp2(lds[2 * cap + a], lds[2 * cap + b], lds[2 * cap + c], lds[2 * cap + e], ly, lx);
    }
    const long long pp = (long long)oy * d.mw + ox;
    float* L = d.logits + n * 3 * oplane + pp;
    L[0] = v0;
    L[oplane] = v1;
    L[2 * oplane] = v2;
    if (d.tn_logits) {
      d.tn_logits[n * 2 * oplane + pp] = v1;
      d.tn_logits[(n * 2 + 1) * oplane + pp] = v2;
    }
    if (aux) {
      const float p = sigmoid_ieee(m);   // of the RESIZED logit (rgb.py:187-194)
      if (d.mask_out) d.mask_out[n * oplane + pp] = m;
      if (d.fg_prob) d.fg_prob[n * oplane + pp] = p;
      if (d.bg_fg_logits) {
        d.bg_fg_logits[n * 2 * oplane + pp] = logf((1.0f - p) + 1e-7f);
        d.bg_fg_logits[(n * 2 + 1) * oplane + pp] = logf(p + 1e-7f);
      }
    }
  }
}

// rows of output per workgroup and the LDS rows that covers (with slack for the device's fused multiply-add)
bool finish_plan(int h, int w, int mh, int mw, int* rows, int* cap_rows) {
  const bool same = mh == h && mw == w;
  long long r = same ? 8 : (8LL * mh) / h;
  if (r < 1) r = 1;
  if (r > mh) r = mh;
  for (;;) {
    const int cap = same ? (int)r : (int)(((r - 1) * (long long)h) / mh) + 4;
    if (3LL * cap * w * 4 <= kFinishLds) {
      *rows = (int)r;
      *cap_rows = cap;
      return true;
    }
    if (r == 1) return false;
    r /= 2;
  }
}

}  // namespace

extern "C" int hiseg_guided_prep_fwd(const hiseg_guided_prep_desc* d, hiseg_stream_t stream) {
  HISEG_REQUIRE(d && d->mask && d->fgp_c && d->N >= 0 && d->h > 0 && d->w > 0, HISEG_ERR_BAD_ARG, "guided_prep: bad args");
  HISEG_REQUIRE(d->dtype == HISEG_F32 || d->dtype == HISEG_BF16, HISEG_ERR_BAD_DTYPE, "guided_prep: unsupported dtype %d",
                d->dtype);
  const int ce = chunk_of(d->dtype);
  HISEG_REQUIRE(d->fgp_cstride >= ce && d->fgp_cstride % ce == 0 && d->fgp_coff >= 0 && d->fgp_coff % ce == 0 &&
                    d->fgp_coff + ce <= d->fgp_cstride && al16(d->fgp_c),
                HISEG_ERR_BAD_SHAPE, "guided_prep: the fg_prob chunk must be 16-byte aligned inside the channel stride");
  HISEG_REQUIRE(d->mask_stride >= (long long)d->h * d->w, HISEG_ERR_BAD_SHAPE, "guided_prep: mask planes overlap");
  const long long P = (long long)d->N * d->h * d->w;
  if (P == 0) return HISEG_OK;
  if (d->dtype == HISEG_BF16)
    hipLaunchKernelGGL(guided_prep_kernel<bf16_t>, dim3(blocks_for(P, kT)), dim3(kT), 0, (hipStream_t)stream, *d);
  else
    hipLaunchKernelGGL(guided_prep_kernel<float>, dim3(blocks_for(P, kT)), dim3(kT), 0, (hipStream_t)stream, *d);
  return hiseg_check_launch("guided_prep");
}

extern "C" int hiseg_guided_attn_fwd(const hiseg_guided_attn_desc* d, hiseg_stream_t stream) {
  HISEG_REQUIRE(d && d->x && d->w1t && d->b1 && d->w2 && d->b2 && d->factor && d->gate && d->P >= 0 && d->C > 0,
                HISEG_ERR_BAD_ARG, "guided_attn: bad args");
  HISEG_REQUIRE(d->dtype == HISEG_F32 || d->dtype == HISEG_BF16, HISEG_ERR_BAD_DTYPE, "guided_attn: unsupported dtype %d",
                d->dtype);
  HISEG_REQUIRE(d->hidden == kHidden, HISEG_ERR_BAD_SHAPE, "guided_attn: hidden width %d (built for %d)", d->hidden, kHidden);
  HISEG_REQUIRE(d->C % chunk_of(d->dtype) == 0 && al16(d->x), HISEG_ERR_BAD_SHAPE, "guided_attn: C must be chunk aligned");
  if (d->P == 0) return HISEG_OK;
  hipStream_t s = (hipStream_t)stream;
  if (d->w1_frag) {
    HISEG_REQUIRE(d->dtype == HISEG_BF16 && d->C == 256 && al16(d->w1_frag), HISEG_ERR_BAD_SHAPE,
                  "guided_attn: the matrix-core form takes bf16 activations with 256 channels");
    const long long groups = (d->P + 15) / 16;
    long long blocks = (groups + 3) / 4;
    if (blocks > 2048) blocks = 2048;   // 8 per CU: the A fragments are loaded once per wave
    hipLaunchKernelGGL(guided_attn_mfma_kernel, dim3((unsigned)blocks), dim3(kT), 0, s, *d);
  } else if (d->dtype == HISEG_BF16) {
    hipLaunchKernelGGL(guided_attn_kernel<bf16_t>, dim3(blocks_for(d->P, kT)), dim3(kT), 0, s, *d);
  } else {
    hipLaunchKernelGGL(guided_attn_kernel<float>, dim3(blocks_for(d->P, kT)), dim3(kT), 0, s, *d);
  }
  return hiseg_check_launch("guided_attn");
}

extern "C" int hiseg_guided_finish_rows(int h, int w, int mh, int mw) {
  int rows = 0, cap = 0;
  if (h <= 0 || w <= 0 || mh <= 0 || mw <= 0 || !finish_plan(h, w, mh, mw, &rows, &cap)) return 0;
  return rows;
}

extern "C" int hiseg_guided_finish_fwd(const hiseg_guided_finish_desc* d, hiseg_stream_t stream) {
  HISEG_REQUIRE(d && d->z && d->w3 && d->b3 && d->logits && d->N >= 0 && d->h > 0 && d->w > 0 && d->C > 0 && d->mh > 0 &&
                    d->mw > 0,
                HISEG_ERR_BAD_ARG, "guided_finish: bad args");
  HISEG_REQUIRE(d->dtype == HISEG_F32 || d->dtype == HISEG_BF16, HISEG_ERR_BAD_DTYPE, "guided_finish: unsupported dtype %d",
                d->dtype);
  HISEG_REQUIRE(d->C % chunk_of(d->dtype) == 0 && al16(d->z), HISEG_ERR_BAD_SHAPE, "guided_finish: C must be chunk aligned");
  const bool aux = d->bg_fg_logits || d->fg_prob || d->mask_out;
  HISEG_REQUIRE(!aux || (d->mask && d->mask_stride >= (long long)d->h * d->w), HISEG_ERR_BAD_ARG,
                "guided_finish: the aux outputs need the mask logits");
  int rows = 0, cap = 0;
  HISEG_REQUIRE(finish_plan(d->h, d->w, d->mh, d->mw, &rows, &cap), HISEG_ERR_BAD_SHAPE,
                "guided_finish: %dx%d -> %dx%d: the source rows of one output row do not fit in LDS", d->h, d->w, d->mh,
                d->mw);
  if (d->N == 0) return HISEG_OK;
  const int tiles = (d->mh + rows - 1) / rows;
  const long long blocks = (long long)d->N * tiles;
  HISEG_REQUIRE(blocks <= 0x7fffffffLL, HISEG_ERR_BAD_SHAPE, "guided_finish: too many workgroups");
  const size_t lds = (size_t)3 * cap * d->w * sizeof(float);
  if (d->dtype == HISEG_BF16)
    hipLaunchKernelGGL(guided_finish_kernel<bf16_t>, dim3((unsigned)blocks), dim3(kT), lds, (hipStream_t)stream, *d, rows,
                       cap, tiles);
  else
    hipLaunchKernelGGL(guided_finish_kernel<float>, dim3((unsigned)blocks), dim3(kT), lds, (hipStream_t)stream, *d, rows,
                       cap, tiles);
  return hiseg_check_launch("guided_finish");
}
