/*
 * hiseg_guided_head.h — the device code of PretrainedUNetGuidedSegmentationHead (advanced/hierarchical_segmentation_rgb.py
 * :43-218, eval mode) that the conv kernels cannot express.  Conventions as in hiseg.h: entry points return a
 * hiseg_status, are stream-ordered, never read device data on the host, never allocate and use no atomics (every output
 * element is written by one thread, so results are bit-reproducible and the calls can be captured in a graph).
 *
 * The head, for ROI features x [N][h][w][C] (channel-last, compute dtype) and the raw foreground logit m f32 of the
 * RoIAligned full-image UNet map (one plane [h][w] per ROI):
 *   p        = 1 / (1 + exp(-m))                        IEEE f32: exp, add, correctly rounded division
 *   a0       = input_adjust(cat(x, p))                  conv kernels, p read as loader source B   (hiseg_guided_prep_fwd)
 *   y        = feature_processor(a0)                    conv kernels
 *   att      = sigmoid(w2 . act(W1 y + b1) + b2)        one value per pixel                       (hiseg_guided_attn_fwd)
 *   gate     = att * (0.5 + 0.5 p)                      y * gate is applied where final_classifier.0 reads y
 *   z        = act(norm(final_classifier.0(y * gate)))  conv kernels, 128 channels
 *   l        = W3 z + b3                                 3 logits per pixel                        (hiseg_guided_finish_fwd)
 *   logits   = resize(l), M = resize(m)                 bilinear, align_corners = False; the identity when the sizes agree
 *   fg_prob  = 1 / (1 + exp(-M))                        the sigmoid AFTER the resize
 *   bg_fg_logits = (log(1 - fg_prob + 1e-7), log(fg_prob + 1e-7))     in f32 with exactly this formula
 *   target_nontarget_logits = logits[:, 1:3], pretrained_bg_fg_mask = M
 *
 * Every descriptor's size is reported by hiseg_guided_struct_sizes; a binding checks its own layout against it.
 */
#ifndef HISEG_GUIDED_HEAD_H_
#define HISEG_GUIDED_HEAD_H_

#include "hiseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Guidance prep: one pass over the mask plane. */
typedef struct hiseg_guided_prep_desc {
  const float* mask;       /* m: plane of ROI n at mask + n * mask_stride, [h][w] contiguous */
  long long mask_stride;   /* floats between the planes of two ROIs (2 h w for channel 1 of an [N][2][h][w] map) */
  int N, h, w;
  int dtype;               /* hiseg_dtype of fgp_c */
  void* fgp_c;             /* p channel-last: pixel q's 16-byte chunk at channel fgp_coff of stride fgp_cstride holds p in
                              its first element and zeros in the rest (loader source B of input_adjust, or channel 256 of
                              a materialised 257-channel input) */
  int fgp_cstride, fgp_coff;
  float* fg_prob;          /* optional: p f32 [N][h][w] */
  float* factor;           /* optional: 0.5 + 0.5 p, f32 [N][h][w] */
} hiseg_guided_prep_desc;

/* Attention gate: 1x1 C -> 64, activation, 1x1 64 -> 1, sigmoid, times the guidance factor. */
typedef struct hiseg_guided_attn_desc {
  int dtype;               /* hiseg_dtype of x */
  const void* x;           /* [P][C] channel-last, channel stride C, C a multiple of the 16-byte chunk */
  long long P;
  int C;
  int hidden;              /* must be 64 */
  const float* w1t;        /* [C][64]: W1 transposed */
  const float* b1;         /* [64] */
  const float* w2;         /* [64] */
  const float* b2;         /* [1] */
  int act;                 /* hiseg_act */
  float act_beta;
  const float* factor;     /* [P] */
  float* att;              /* optional: the raw attention map [P] */
  float* gate;             /* att * factor [P] */
  const void* w1_frag;     /* optional, bf16 x only: W1 as bf16 MFMA A-operand fragments [tile 4][kstep C/32][lane 64][8],
                              element j of lane l = W1[16 tile + (l & 15)][32 kstep + 8 (l >> 4) + j]; the matrix-core
                              form of the kernel runs when it is given (C a multiple of 32) */
} hiseg_guided_attn_desc;

/* Finish: 1x1 C -> 3 at ROI size, bilinear resize to mask size, NCHW f32 logits and the aux tensors. */
typedef struct hiseg_guided_finish_desc {
  int dtype;               /* hiseg_dtype of z */
  const void* z;           /* [N][h][w][C] channel-last, channel stride C, C a multiple of the 16-byte chunk */
  int N, h, w, C;
  const float* w3;         /* [3][C] */
  const float* b3;         /* [3] */
  int mh, mw;              /* mask size */
  float* logits;           /* [N][3][mh][mw] */
  const float* mask;       /* m as in the prep descriptor; read only when an aux output is asked for */
  long long mask_stride;
  float* bg_fg_logits;     /* optional aux outputs (NULL to skip): [N][2][mh][mw] */
  float* fg_prob;          /*   [N][mh][mw] */
  float* mask_out;         /*   [N][mh][mw] */
  float* tn_logits;        /*   [N][2][mh][mw] */
} hiseg_guided_finish_desc;

/* Sizes of the three descriptors above, in declaration order; returns how many there are. */
int hiseg_guided_struct_sizes(long long* out, int n);

int hiseg_guided_prep_fwd(const hiseg_guided_prep_desc* d, hiseg_stream_t stream);
int hiseg_guided_attn_fwd(const hiseg_guided_attn_desc* d, hiseg_stream_t stream);

/* Output rows one workgroup of the finish kernel owns (>= 1), or 0 when the logits of the source rows a single
 * output row needs do not fit in LDS (the call then fails with HISEG_ERR_BAD_SHAPE). */
int hiseg_guided_finish_rows(int h, int w, int mh, int mw);
int hiseg_guided_finish_fwd(const hiseg_guided_finish_desc* d, hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
