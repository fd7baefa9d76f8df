// The target branch's last 1x1 conv (Ct -> 2, refinement.py:521) over K consecutive channels of one pixel.
// hier_combine_kernel (misc.hip) and conv_hwc_kernel's head2 epilogue (conv_hwc.hip) both walk a pixel's channels in
// ascending order through this one function, starting from the bias, so both get the same contraction of the
// multiply-add and the two paths agree bit for bit.
#pragma once
#include "common.h"

namespace hiseg {

// w0 / w1: the two output rows' weights of these K channels; v: the channels' values (bf16 widened, or f32)
template <int K>
__device__ __forceinline__ void head2_acc(float& t0, float& t1, const float* w0, const float* w1, const float (&v)[K]) {
#pragma unroll
  for (int e = 0; e < K; ++e) {
    t0 += w0[e] * v[e];
    t1 += w1[e] * v[e];
  }
}

}  // namespace hiseg
