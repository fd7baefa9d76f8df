/*
 * hiseg_compose.h — full-frame instance composition on the GPU: the consumer stage of the reference's serving
 * script (test_hierarchical_instance_peopleseg_onnx.py), which turns per-ROI outputs into one label map and one
 * colour overlay per frame on the host, one ROI at a time.  Conventions as in hiseg.h.
 *
 * Packed masks.  A ROI's target mask is carried between the entry points as bits: mh rows of
 * hiseg_compose_words_per_row(mw) = (mw + 31) / 32 32-bit words, pixel j of a row is bit (j & 31) of word (j >> 5),
 * padding bits are 0.  N ROIs are N * mh * words_per_row contiguous words.
 *
 * Every result is a pure function of its inputs: no atomics, fixed reduction trees, every output element written
 * once.  A problem with no output element (N == 0 for the front ends, B * H * W == 0 for the frame passes) returns
 * HISEG_OK without a launch and its pointers may be null; mh * mw == 0, a negative count or a null pointer of a
 * non-empty problem is HISEG_ERR_BAD_ARG before any launch.
 */
#ifndef HISEG_COMPOSE_H_
#define HISEG_COMPOSE_H_

#include "hiseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host function (no GPU): 32-bit words per packed mask row, (mw + 31) / 32; 0 for mw <= 0. */
int hiseg_compose_words_per_row(int mw);

/* process_mask_output, per-ROI half (test_hierarchical_instance_peopleseg_onnx.py:249-263, 281): logits f32
 * [N][3][mh][mw] (NCHW) -> bits, score f32 [N], count i32 [N].  A pixel is set when the first maximum of the three
 * classes (np.argmax) is class 1 and the f32 softmax maximum, 1 / sum(exp(l - max)), is > score_threshold.
 * count = set pixels; score = mean of the softmax maximum over them, 0 when there is none.  One workgroup per
 * ROI; the score is summed per lane in pixel order, then through a fixed 256-lane tree.  NaN logits are out of scope
 * (a NaN is never the maximum here). */
int hiseg_roi_mask_classify_fwd(const float* logits, long long N, int mh, int mw, float score_threshold,
                                unsigned int* bits, float* score, int* count, hiseg_stream_t stream);

/* The same outputs from the exported contract's instance_masks f32 [N][1][mh][mw] (the model's own argmax == 1
 * planes, hiseg_instance_masks_fwd, possibly post-filtered): a pixel is set when its value is > 0.5; score = 1 if
 * any pixel is set, else 0. */
int hiseg_roi_mask_pack_fwd(const float* masks, long long N, int mh, int mw, unsigned int* bits, float* score,
                            int* count, hiseg_stream_t stream);

/* process_mask_output, box half (:265-278), and the paint loop of visualize_instance_segmentation (:362-385) as a
 * label map: bits, score f32 [N], rois f32 [N][5] (batch index, x1, y1, x2, y2 normalised) -> label i32 [B][H][W],
 * 0 = background, k + 1 = ROI k of `rois` owns the pixel.  (H, W) is the frame the boxes are scaled to -- the
 * original image, not necessarily the model's input.
 *   box   = [int(x1 * W), int(y1 * H), int(x2 * W), int(y2 * H)], each product in f32 (np.float32 times a Python
 *           int), truncated toward zero (denormalize_bbox, :144-161); a product beyond +-1e9 is clamped there and a
 *           NaN makes the ROI paint nothing
 *   skip  : x2 <= x1 or y2 <= y1 in pixels (:272), score <= 0 (:367), batch index != the frame's
 *   inside: cv2.resize(mask, (bw, bh), INTER_NEAREST): source column min(floor(dx * (1.0 / (bw / (double)mw))),
 *           mw - 1) for dx = x - box.x1, rows likewise
 *   owner : the highest ROI index of the frame whose resized mask is set at the pixel (the later ROI repaints)
 * rois need not be sorted by batch index, and N is unbounded.  A box that reaches outside the frame is clipped to
 * it with the mask still mapped over the unclipped box; the reference raises there (its slice assignment does not
 * broadcast).  Kernel form: a gather.  One workgroup per 128 x 8 frame tile scans the ROIs from the highest index
 * down in chunks of 64, keeps those of its frame whose box meets the tile in index order (wave ballot compaction
 * into LDS), and every pixel walks that list from the back to its first hit; the tile stops once every pixel has an
 * owner.  Each label is written once, four to a 16-byte store where W is a multiple of 4. */
int hiseg_instance_map_fwd(const unsigned int* bits, const float* score, const float* rois, long long N, int mh,
                           int mw, int B, int H, int W, int* label, hiseg_stream_t stream);

/* The blend of visualize_instance_segmentation (:377-400): label i32 [B][H][W], image u8 [B][H][W][3], colors u8
 * [N][3] -> out u8 [B][H][W][3] = cv2.addWeighted(image, 1 - alpha, overlay, alpha, 0) with overlay = colors[label
 * - 1], or 0 where label is 0 (pixels nobody owns are dimmed by 1 - alpha, as in the reference).  The weights are
 * (float)(1.0 - alpha) and (float)alpha; per byte saturate(round_half_even(image * w_image + overlay * w_overlay)),
 * two f32 products and one f32 sum, no fused multiply-add.  A label outside [0, N] is read as 0.  image and out are
 * distinct buffers. */
int hiseg_instance_overlay_fwd(const int* label, const unsigned char* image, const unsigned char* colors, long long N,
                               int B, int H, int W, double alpha, unsigned char* out, hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
