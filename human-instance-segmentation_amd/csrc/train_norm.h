// What bn_train.hip, ln_train.hip and train_ew.hip share (each piece is used by at least two of them), the type
// dispatch they share with the head's training files (attn_spatial_train.hip, channel_gate_train.hip, ubf_train.hip),
// and the one declaration each of bn_finalize_splits and sum_rows.
#pragma once
#include "common.h"
#include "hiseg_train.h"

namespace hiseg {

template <typename T>
__device__ __forceinline__ float ld(const void* p, long long i) { return Elem<T>::load(p, i); }
template <typename T>
__device__ __forceinline__ void st(void* p, long long i, float v) { Elem<T>::store(p, i, v); }

__device__ __forceinline__ float act_grad(float y, int act) {
  switch (act) {
    case HISEG_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case HISEG_ACT_SIGMOID: return y * (1.f - y);
    default: return 1.f;
  }
}

// One 16-B chunk (8 bf16 / 4 f32 channels) as f32 values.
template <typename T>
__device__ __forceinline__ void ldv(const void* p, long long i, float* v) {
  Chunk<T>::unpack(*reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p) + i), v);
}
template <typename T>
__device__ __forceinline__ void stv(void* p, long long i, const float* v) {
  *reinterpret_cast<uint4*>(reinterpret_cast<T*>(p) + i) = Chunk<T>::pack(v);
}

// Grid of the scalar element-wise passes: blocks of 256 elements, capped (the kernels stride).
inline unsigned ew_blocks(long long n) {
  long long b = (n + 255) / 256;
  return (unsigned)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

// 16-B chunk path eligibility: channel count, strides and offsets in whole chunks, aligned base.
inline bool vec_ok(int dtype, int C, const void* p, int cs, int coff) {
  const int v = dtype == HISEG_BF16 ? 8 : 4;
  return p == nullptr || (C % v == 0 && cs % v == 0 && coff % v == 0 && al16(p));
}

// Grid of the chunk element-wise passes: pixel-row blocks (<= 2048 -> 8 waves per SIMD), channel groups in y.
inline dim3 vec_grid(long long P, int C, int dtype) {
  const int nch = C / (dtype == HISEG_BF16 ? 8 : 4);
  const int ct = nch < 256 ? nch : 256, R = 256 / ct;
  long long bx = (P + R - 1) / R;
  if (bx > 2048) bx = 2048;
  return dim3((unsigned)(bx < 1 ? 1 : bx), (unsigned)((nch + 255) / 256));
}

}  // namespace hiseg

// Run the statement(s) with T = bf16_t or float.  (misc.hip and se_gate.hip keep their own (dtype, KERNEL, ...) form.)
#define DISPATCH_T(dtype, ...)                       \
  do {                                               \
    if ((dtype) == HISEG_BF16) {                     \
      using T = hiseg::bf16_t;                       \
      __VA_ARGS__;                                   \
    } else {                                         \
      using T = float;                               \
      __VA_ARGS__;                                   \
    }                                                \
  } while (0)

// bn_train.hip: the BatchNorm statistics merge over an explicit split count, rows `rs` floats apart (0: 3 C).
int bn_finalize_splits(const float* partial, int S, int C, long long P, const float* gamma, const float* beta,
                       float eps, float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                       float* scale, float* shift, hipStream_t stream, long long rs = 0);

// ubf_train.hip: out[c] (+)= sum_r part[r*ld + c], c < cols.  Consumes part (scratch) when rows > 64.
namespace hiseg { void sum_rows(float* part, int rows, int ld, int cols, float* out, int acc, hipStream_t s); }
