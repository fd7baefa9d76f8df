/*
 * hiseg_kd.h — teacher -> student knowledge-distillation term of the ROI model
 * (advanced/knowledge_distillation.py:94-125, DistillationLoss.forward, and its gradient w.r.t. the student's
 * tensors).  Conventions as in hiseg.h: entry points return a hiseg_status, are stream-ordered, never read device
 * data on the host and never allocate; the workspace size (in floats) comes from hiseg_kd_ws.  No kernel uses an
 * atomic: every sum is a block partial added in a fixed order by a finalize kernel that accumulates in double, so
 * results are bit-identical from run to run.
 *
 * Heads, f32 NCHW, student and teacher of the same shape:
 *   head 0  logits            [N][3][H][W]   weight 1     (student null: the head is off, distill_logits=False)
 *   head 1  bg_fg             [N][2][H][W]   weight 0.3   (both null: absent)
 *   head 2  target_nontarget  [N][2][H][W]   weight 0.3   (both null: absent)
 * Per head with weight w and temperature T (nn.KLDivLoss('batchmean') of log_softmax(s / T) against
 * softmax(t / T), times T^2):
 *   q = softmax(t / T),  ls = log_softmax(s / T)               (per pixel, f32, max subtracted)
 *   term = w * T^2 * (1 / N) * sum over n, c, y, x of (xlogy(q, q) - q * ls)
 * A teacher probability that underflows to 0 contributes 0.
 * T: *dev_T (device scalar) when dev_T is non-null, else the host argument T (> 0).
 */
#ifndef HISEG_KD_H_
#define HISEG_KD_H_

#include "hiseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HISEG_KD_NOUT 4 /* floats of the output vector */

/* Workspace of hiseg_kd_loss_fwd in floats (8-byte aligned base required). */
long long hiseg_kd_ws(int N, int H, int W);

/* out[0] = sum of the enabled terms, out[1], out[2], out[3] = the terms of heads 0, 1, 2 (0 where the head is
 * off).  One launch covers the three heads, a second one adds the block partials. */
int hiseg_kd_loss_fwd(const float* s_logits, const float* t_logits, const float* s_bgfg, const float* t_bgfg,
                      const float* s_tn, const float* t_tn, int N, int H, int W, float T, const float* dev_T,
                      float* ws, float* out, hiseg_stream_t stream);

/* d<head> = *gscale (device scalar) * d out[0] / d s<head> = *gscale * w * T / N * (softmax(s / T) - q), for
 * every head whose student pointer is non-null (its teacher and gradient pointers are then required).  Recomputed
 * from the logits: the backward reads nothing the forward left behind, so it needs no workspace. */
int hiseg_kd_loss_bwd(const float* s_logits, const float* t_logits, const float* s_bgfg, const float* t_bgfg,
                      const float* s_tn, const float* t_tn, int N, int H, int W, float T, const float* dev_T,
                      const float* gscale, float* d_logits, float* d_bgfg, float* d_tn, hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HISEG_KD_H_ */
