/*
 * hiseg_refine.h — the boundary refinement stage of the hierarchical head and the active-contour loss term
 * (advanced/hierarchical_segmentation_refinement.py: BoundaryRefinementModule :58-149, active_contour_loss
 * :347-386).  Conventions as in hiseg.h: entry points return a hiseg_status, are stream-ordered, never read
 * device data on the host and never allocate; workspace sizes (in floats) come from the *_ws queries.
 *
 * The stage, for logits x f32 [N][3][H][W] (NCHW, contiguous), H >= 2 and W >= 2 (else HISEG_ERR_BAD_ARG):
 *   p  = softmax(x, 1)
 *   dy = |p[h+1] - p[h]|, dx = |p[w+1] - p[w]|, the last row / column a replicate of the one before it
 *   e  = mean_c sqrt(dy^2 + dx^2)                                     (e_raw [N][H][W])
 *   mn, mx = min / max of e over the WHOLE [N][H][W] tensor           (mnmx [2], device memory)
 *   E  = 0 where mx - mn < 1e-6, else (e - mn) / (mx - mn + 1e-6)
 *   out = x + blend * R * E        R = edge_conv(x), f32 channel-last [N][H][W][r_cstride], 3 real channels
 * The convolutions of edge_conv run on the library's conv kernels between hiseg_edge_map_fwd and
 * hiseg_boundary_blend_fwd.
 *
 * The backward differentiates through everything, as the reference's autograd does: the softmax, the padded
 * differences (the difference before the last row / column receives the gradient of two rows / columns), the sqrt
 * and the global min and max (the gradient of Tensor.min() / .max() goes to the extremal elements, split evenly
 * over ties).  It is computed in plain IEEE f32 with no special case at zero: where dy = dx = 0 exactly for a class
 * the sqrt's backward is 0/0 and the NaN reaches dx at that pixel and its +1 neighbours, as in the reference.
 * Every kernel is in gather form (no floating-point atomics); the reductions are block partials summed in a fixed
 * order, so results are bit-reproducible from run to run.
 */
#ifndef HISEG_REFINE_H_
#define HISEG_REFINE_H_

#include "hiseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of hiseg_edge_map_fwd, in floats (block partials of the min / max). */
long long hiseg_edge_map_ws(int N, int H, int W);

/* e_raw [N][H][W] and mnmx [2] from x.  Optional outputs (NULL to skip): probs [N][3][H][W], the softmax the
 * backward reads; x_cl, the channel-last copy of x in the compute dtype cl_dtype (hiseg_dtype) with channel stride
 * cl_cstride >= 3 (channels >= 3 written as zero) that the conv path takes. */
int hiseg_edge_map_fwd(const float* x, int N, int H, int W, float* e_raw, float* mnmx, float* probs, void* x_cl,
                       int cl_dtype, int cl_cstride, float* ws, hiseg_stream_t stream);

/* out [N][3][H][W] = x + blend * R * E; mn, mx and blend (a 0-dim parameter) are read on the device and the
 * mx - mn < 1e-6 branch is taken there.  E_out (optional) [N][H][W] receives the normalised edge map. */
int hiseg_boundary_blend_fwd(const float* x, const float* R, int r_cstride, const float* e_raw, const float* mnmx,
                             const float* blend, int N, int H, int W, float* out, float* E_out,
                             hiseg_stream_t stream);

/* The whole stage after hiseg_edge_map_fwd in one kernel, for the common inference case: both norms eval BatchNorm
 * folded into per-channel (scale, shift) with the conv bias, ReLU, 32 edge channels, bf16 intermediates.  A workgroup
 * owns a 16 x 16 tile: the logit tile with a halo of 2 and conv1's output (VALU, K = 27, f32 weights w1
 * [32][ci * 9 + ky * 3 + kx]) stay in LDS, the latter as bf16; conv2 runs on MFMA (K = 288) with w2_frag, the bf16
 * weights in fragment order [tap ky * 3 + kx][tile][lane][8]: element j of lane l of tile t is
 * w2[co = 16 t + (l & 15)][ci = 8 (l >> 4) + j][ky][kx]; the 1x1 (w3 [3][32], b3 [3]) and the blend run in registers.
 * out [N][3][H][W] f32.  Anything else takes the conv kernels between the edge map and the blend. */
int hiseg_boundary_refine_fused(const float* x, int N, int H, int W, const float* e_raw, const float* mnmx,
                                const float* blend, const float* w1, const float* scale1, const float* shift1,
                                const void* w2_frag, const float* scale2, const float* shift2, const float* w3,
                                const float* b3, float* out, hiseg_stream_t stream);

/* Workspace shared by hiseg_boundary_blend_bwd and hiseg_edge_map_bwd, in floats. */
long long hiseg_boundary_bwd_ws(int N, int H, int W);

/* From g = d loss / d out [N][3][H][W]: dR [N][H][W][dr_cstride] (3 channels written, the rest zero), *dblend +=
 * sum g R E, and in ws the per-pixel d loss / d E with the global sums sum dE, sum dE (e - mn) and the tie counts of
 * the min and the max that hiseg_edge_map_bwd needs. */
int hiseg_boundary_blend_bwd(const float* g, const float* R, int r_cstride, const float* e_raw, const float* mnmx,
                             const float* blend, int N, int H, int W, float* dR, int dr_cstride, float* dblend,
                             float* ws, hiseg_stream_t stream);

/* dx [N][3][H][W] = g + g_cl + (the gradient through E), with g_cl (optional) the gradient the conv path left on
 * the channel-last copy of x (cl_dtype, cl_cstride) and ws as hiseg_boundary_blend_bwd left it. */
int hiseg_edge_map_bwd(const float* g, const void* g_cl, int cl_dtype, int cl_cstride, const float* probs,
                       const float* e_raw, const float* mnmx, int N, int H, int W, float* ws, float* dx,
                       hiseg_stream_t stream);

/* active_contour_loss(softmax(pred, 1)) with smoothness_weight 0.01, pred f32 [N][3][H][W], H >= 2 and W >= 2:
 * mean min(|dy|, 10) + mean min(|dx|, 10) + 0.01 (mean |ddy| + mean |ddx|) of the class-1 probability; a
 * curvature term is 0 when its axis has fewer than 3 samples.  out[0] = min(loss, 10) (the clamp of
 * RefinedHierarchicalLoss), out[1] = loss.  The forward leaves what the backward needs in ws. */
long long hiseg_active_contour_ws(int N, int H, int W);
int hiseg_active_contour_fwd(const float* pred, int N, int H, int W, float* ws, float* out, hiseg_stream_t stream);
/* dpred [N][3][H][W] = *gscale (device scalar) * d out[0] / d pred. */
int hiseg_active_contour_bwd(const float* pred, int N, int H, int W, const float* ws, const float* gscale,
                             float* dpred, hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
