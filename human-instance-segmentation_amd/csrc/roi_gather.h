// The fused 3-class ROI target gather (include/hiseg_data.h), shared by hiseg_roi_targets (data.hip) and its
// flipped form hiseg_roi_targets_flip (augment.hip).
#pragma once
#include <math.h>

#include "common.h"
#include "hiseg_data.h"

namespace hiseg {

// cv2.resize(..., INTER_NEAREST) source index (OpenCV resizeNN): min(floor(x / (dst / src)), src - 1)
__device__ __forceinline__ int nn_src(int x, int src, int dst) {
  const double ifx = 1.0 / ((double)dst / (double)src);
  const int s = (int)floor((double)x * ifx);
  return s < src - 1 ? s : src - 1;
}

// Class id of output pixel idx = i * mw + j of sample d.  flip: d's ROI is the box of the mirrored image, and
// ROI column c is image column img_w - 1 - (x1 + c) of the unmirrored instance masks (dataset.py:180-212).
__device__ __forceinline__ long long roi_target_class(const uint8_t* masks, const hiseg_roi_target_desc& d, int mh,
                                                      int mw, int idx, bool flip) {
  const int i = idx / mw, j = idx - (idx / mw) * mw;
  const int rh = d.y2 - d.y1, rw = d.x2 - d.x1;
  const int yi = d.y1 + nn_src(i, rh, mh);                                     // dataset.py:272 (ROI -> mask)
  int xi = d.x1 + nn_src(j, rw, mw);
  if (flip) xi = d.img_w - 1 - xi;
  const int y0 = nn_src(yi, d.h0, d.img_h), x0 = nn_src(xi, d.w0, d.img_w);  // dataset.py:117 (orig -> image)
  const long long plane = (long long)d.h0 * d.w0;
  const uint8_t* m = masks + d.mask_offset + (long long)y0 * d.w0 + x0;
  if (m[(long long)d.target * plane] > 0) return 1;                           // dataset.py:153
  for (int k = 0; k < d.n_inst; ++k)
    if (k != d.target && m[(long long)k * plane] > 0) return 2;               // dataset.py:156-160
  return 0;
}

}  // namespace hiseg
