/*
 * hiseg_metrics.h — validation metrics of the ROI masks on the GPU (train_utils.py:109-402, evaluate_model;
 * the per-sample IoU and confusion loops of :279-318 over calculate_iou :14-22 and
 * calculate_confusion_matrix :25-47).  Conventions as in hiseg.h.
 *
 * The reference moves the predicted classes to the host and counts them with one boolean reduction (and
 * one .item()) per (sample, class) and per (sample, target, prediction) pair.  Every metric it reports is
 * a function of one small per-sample histogram, so one HBM pass builds that histogram for all samples:
 *
 *   conf[n][t][p] += #{ pixels of sample n with target row t and predicted column p }
 *
 * rows    t = target value for 0 <= target < C;  t = C for target >= C;  t = C+1 for target < 0
 * columns p = predicted class (argmax over the C logits: first maximum, NaN counts as the maximum,
 *             as torch.argmax), or for class-label input p = label for 0 <= label < C, p = C otherwise
 *
 * so that the IoUs (pred == c vs target == c), the 3x3 confusion matrix, the background-vs-target matrix
 * (target == 1 vs pred == 1, every other target value counting as background) and the target-vs-nontarget
 * matrix over target > 0 are all exact sums of conf entries.
 */
#ifndef HISEG_METRICS_H_
#define HISEG_METRICS_H_

#include "hiseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Accumulates into conf (uint64, [N][C+2][C+1], zeroed by the caller for a fresh count).
 *   logits       [N][C][HW] (NCHW) of dtype HISEG_F32 or HISEG_BF16, or null when pred_labels is given
 *   pred_labels  int64 [N][HW] predicted class ids (used when logits is null)
 *   target       int64 [N][HW]
 * 2 <= C <= 4.  Reads 4*C (f32) + 8 bytes per pixel once; no host synchronisation. */
int hiseg_seg_confusion(const void* logits, int dtype, const long long* pred_labels, const long long* target,
                        int N, int C, long long HW, unsigned long long* conf, hiseg_stream_t stream);

/*
 * Distillation validation (train_distillation_staged.py:369-581, evaluate): student mIoU, teacher mIoU and
 * teacher-student agreement of the binary UNet pair.  The reference builds them from about 40 elementwise and
 * reduction passes over [B,1,H,W] per batch; every one of those numbers is a function of eight counts per
 * sample, the joint histogram of the three bits (mask, teacher, student):
 *
 *   counts[b][4*m + 2*t + s] += #{ pixels of sample b with mask bit m, teacher bit t, student bit s }
 *
 * Foreground predicate of a logit x (the reference's `sigmoid(x) > 0.5`, :444-446):
 *
 *   bit(x) = x > 0x1.8p-24f        (1.5 * 2^-24, about 8.94e-8; compared in f32)
 *
 * which is `1.0f / (1.0f + expf(-x)) > 0.5f` with every f32 operation correctly rounded: the quotient exceeds
 * 0.5 iff fl(1 + fl(exp(-x))) < 2, 1 + (1 - 2^-24) ties to the even 2.0, so fl(exp(-x)) <= 1 - 2^-23 is
 * needed, i.e. exp(-x) below the midpoint 1 - 1.5 * 2^-24, i.e. x > 1.5 * 2^-24 (x = 1.5 * 2^-24 itself gives
 * exp(-x) just above that midpoint).  So 0.0, -0.0, every negative value, NaN and 2^-24 are background; 2^-23,
 * every x >= 1e-6 and +inf are foreground.  Inside the open band (0, 1e-6) a sigmoid whose exp is not
 * correctly rounded may answer differently (torch's CPU and GPU kernels are such implementations): no parity
 * is claimed there.  bf16 logits are widened to f32 and then compared; torch's bf16 sigmoid rounds its result
 * to bf16 first, where 0.5 + 2^-9 is the first value above 0.5, so torch on bf16 logits calls small positive
 * logits background that this predicate (and the reference's f32 path) calls foreground.
 *
 * A mask pixel is foreground iff mask > 0.5 (:449; NaN is background; any non-zero uint8 is foreground).
 */
enum { HISEG_U8 = 2 };   /* mask dtype of hiseg_binary_seg_stats (beside HISEG_F32) */

/* Accumulates into counts (uint64, [B][8], zeroed by the caller for a fresh count).
 *   student  [B][HW] logits, s_dtype HISEG_F32 or HISEG_BF16
 *   teacher  [B][HW] logits, t_dtype HISEG_F32 or HISEG_BF16; null: t = s (the reference's teacher-less
 *            mode, :445-448), t_dtype ignored
 *   mask     [B][HW], m_dtype HISEG_F32 or HISEG_U8
 * B <= 65535.  One pass, 12 bytes per pixel for f32 inputs; integer counts, so the result is exact and
 * independent of the launch shape; no host synchronisation. */
int hiseg_binary_seg_stats(const void* student, int s_dtype, const void* teacher, int t_dtype,
                           const void* mask, int m_dtype, int B, long long HW, unsigned long long* counts,
                           hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
