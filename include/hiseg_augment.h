/*
 * hiseg_augment.h — ROI-safe training augmentation on the GPU (src/human_edge_detection/augmentations.py:158-257
 * get_roi_safe_light_transforms / get_roi_safe_heavy_transforms as installed by train_advanced.py:1031-1049, and
 * dataset.py:172-212 for the ROI box and ROI mask of a flipped sample).  Conventions as in hiseg.h.
 *
 * The host draws the random parameters and turns every colour transform into 8-bit tables (two tables in a row
 * compose exactly into one) and every blur into a ksize x ksize correlation kernel; one launch then applies, per
 * sample and on 8-bit values, in the order of the reference's Compose:
 *   1. horizontal flip                       p[y][x] = src[y][flip ? W-1-x : x]
 *   2. HSV round trip (if hsv)               cv2's 8-bit RGB2HSV, hsv_lut per channel, cv2's 8-bit HSV2RGB
 *   3. channel tables                        c = rgb_lut[ch][c]
 *   4. filter (if ksize)                     correlation with kernel, reflect-101 border, f32 sum in row-major
 *                                            tap order, clamp(rint(sum), 0, 255); it sees the flipped pixels, so
 *                                            an asymmetric kernel is not mirrored
 *   5. store                                 out[b][ch][y][x] = out_table[value]   (Normalize / ToTensor)
 *
 * albumentations and cv2 are restated, unpinned: the arithmetic (the 12-bit fixed-point sdiv / hdiv tables of
 * RGB2HSV, the f32 sector form of HSV2RGB without FMA contraction, reflect-101) follows their published sources
 * but has not been compared against the libraries themselves.
 */
#ifndef HISEG_AUGMENT_H_
#define HISEG_AUGMENT_H_

#include "hiseg.h"
#include "hiseg_data.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiseg_aug_sample {
  int flip;                        /* 0/1 horizontal flip */
  int hsv;                         /* 0/1 run the HSV round trip through hsv_lut */
  int ksize;                       /* 0 (no filter), 3, 5 or 7 */
  int reserved;
  unsigned char hsv_lut[3][256];   /* H, S, V tables (H indexed 0..179) */
  unsigned char rgb_lut[3][256];   /* per-channel table applied after the HSV stage */
  float kernel[49];                /* row-major ksize x ksize correlation weights */
} hiseg_aug_sample;

/* sizeof(hiseg_aug_sample) as compiled, for a binding to check its mirror against. */
int hiseg_aug_struct_size(void);

/* Host function (no GPU): checks B packed samples in HOST memory -- ksize in {0, 3, 5, 7}, flip and hsv 0 or 1 --
 * and returns HISEG_OK or HISEG_ERR_BAD_ARG. */
int hiseg_aug_validate(const hiseg_aug_sample* host_samples, int B);

/* src 8-bit [B][H][W][3]; samples: device array [B]; out_table: device f32[256]; out f32 [B][3][H][W].
 * One launch, no atomics, no host synchronisation (graph-capturable).  Null pointers and H or W < 4 (the
 * reflect border of a 7 x 7 needs 4) are refused.  The samples live on the device, so the entry point cannot
 * read their ksize without a synchronisation: hiseg_aug_validate refuses a ksize outside {0, 3, 5, 7} on the
 * host copy before it is uploaded (hiseg.augment.AugParams calls it), and the kernel runs such a sample
 * without the filter. */
int hiseg_augment_fwd(const unsigned char* src, const hiseg_aug_sample* samples, const float* out_table, int B,
                      int H, int W, float* out, hiseg_stream_t stream);

/* hiseg_roi_targets with a per-sample horizontal flip (flip: device int[B]).  A flipped sample's desc carries
 * the ALREADY FLIPPED box (x1', x2') = (img_w - x2, img_w - x1); output pixel (oy, ox) reads ROI column cx
 * through the same nearest map and then the image column img_w - 1 - (x1' + cx): the reference's "pad the ROI
 * mask to the full image, flip, crop at the new box" (dataset.py:180-212).  flip[b] == 0: hiseg_roi_targets. */
int hiseg_roi_targets_flip(const unsigned char* masks, const hiseg_roi_target_desc* descs, const int* flip, int B,
                           int mh, int mw, long long* out, hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
