/*
 * hiseg_distance.h — exact Euclidean boundary distance transform, boundary weight map and the distance-aware
 * segmentation loss (advanced/distance_aware_loss.py: DistanceTransform.compute_boundary_distance :13-50,
 * BoundaryWeightGenerator.generate_weights :147-185, DistanceAwareSegmentationLoss.forward :238-310; losses.py
 * DiceLoss :9-88, FocalLoss :91-127).  Conventions as in hiseg.h: entry points return a hiseg_status, are
 * stream-ordered, never read device data on the host and never allocate; workspace sizes (in floats) come from
 * hiseg_distance_ws.  No kernel uses an atomic: every sum is a block partial added in a fixed order, so results
 * are bit-identical from run to run.
 *
 * Site set of a sample (target int64 [N][H][W], values 0, 1, 2), decided per sample:
 *   all three values present : pixel (y, x) is a site when it differs from (y-1, x) (y >= 1) or (y, x-1) (x >= 1)
 *   otherwise                : the pixels equal to 1
 *   no site at all           : one virtual site at row -1, column 0 (d2 = (y+1)^2 + x^2), what scipy 1.15.3's
 *                              distance_transform_edt returns for an input without background
 * d2 [N][H][W] int32 = min(squared Euclidean distance to the nearest site, d2cap).  Only sites with
 * |dy|, |dx| <= radius are searched, so d2 is exact wherever the true distance is <= radius and d2cap elsewhere
 * provided d2cap <= (radius + 1)^2.
 *
 * A sample runs in one workgroup with its mask and row distances in LDS while hiseg_distance_resident(H, W); above
 * that a halo-tiled variant (64 x 64 tiles, radius <= HISEG_DISTANCE_MAX_HALO) runs.  H, W <= 16384.
 */
#ifndef HISEG_DISTANCE_H_
#define HISEG_DISTANCE_H_

#include "hiseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HISEG_DISTANCE_NOUT 8      /* floats of the loss output vector (5 used) */
#define HISEG_DISTANCE_MAX_HALO 32 /* largest radius of the halo-tiled variant */

/* 1 when an H x W mask takes the LDS-resident kernel, 0 when it takes the halo-tiled one. */
int hiseg_distance_resident(int H, int W);

/* Workspace of every entry point below, in floats (8-byte aligned base required). */
long long hiseg_distance_ws(int N, int H, int W);

/* d2 from target.  force_tiled != 0 takes the halo-tiled variant at any size (tests).  HISEG_ERR_BAD_SHAPE when
 * the mask is not resident and radius > HISEG_DISTANCE_MAX_HALO. */
int hiseg_distance_transform(const long long* target, int N, int H, int W, int radius, int d2cap, int force_tiled,
                             int* d2, float* ws, hiseg_stream_t stream);

/* d2 (radius width - 1, cap width^2) and the weight map [N][H][W] f32:
 *   w = f32(1 + (boundary_weight - 1) * table[d2]) where d2 < width^2, else 1         (evaluated in double)
 *   w = w * instance_sep_weight (f32) where inst_present[n] and inst_dist[n][y][x] < 50
 * table: device double [width^2], (1 - sqrt(d2) / width) built by the caller.  dev_weights (optional): device
 * float [2] = {boundary_weight, instance_sep_weight}, read on the device in place of the two host arguments.
 * inst_dist (optional) f32 [N][H][W] with inst_present uint8 [N]. */
int hiseg_distance_weight_map(const long long* target, int N, int H, int W, int width, const double* table,
                              double boundary_weight, double instance_sep_weight, const float* dev_weights,
                              const float* inst_dist, const unsigned char* inst_present, int force_tiled, int* d2,
                              float* weights, float* ws, hiseg_stream_t stream);

/* Loss forward on logits pred f32 [N][3][H][W]:
 *   ce      = per-pixel cross entropy;  wce = mean(ce * w)
 *   focal   : F = mean(alpha_t (1 - p_t)^gamma ce), p_t = exp(-ce), alpha = class_weights or 1;  wce = F * mean(w)
 *   class_weights (optional, device float [3]) : wce *= mean(class_weights[target])   (in both forms)
 *   dice    = mean_n (1 - (2 sum p1 t1 + 1e-6) / (sum p1 + sum t1 + 1e-6)), class 1 only
 * out[0] = ce_weight * wce + dice_weight * dice, out[1] = wce, out[2] = dice, out[3] = accuracy of argmax(pred)
 * (ties to the lowest class) over the pixels with w > 1.5 (0 when there are none), out[4] = mean(w).  The forward
 * leaves the backward's coefficients in ws. */
int hiseg_distance_loss_fwd(const float* pred, const long long* target, const float* weights, int N, int H, int W,
                            const float* class_weights, int use_focal, float focal_gamma, float ce_weight,
                            float dice_weight, float* ws, float* out, hiseg_stream_t stream);

/* dpred [N][3][H][W] = *gscale (device scalar) * d out[0] / d pred, with ws as the forward left it. */
int hiseg_distance_loss_bwd(const float* pred, const long long* target, const float* weights, int N, int H, int W,
                            const float* class_weights, int use_focal, float focal_gamma, const float* ws,
                            const float* gscale, float* dpred, hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
