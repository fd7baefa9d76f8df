/*
 * hiseg_post.h — mask post-processing on the GPU: the clean-up stage the reference runs on the exported
 * instance / binary masks (src/human_edge_detection/edge_smoothing.py, bilateral_filter.py; exported as separate
 * graphs by export_edge_smoothing_onnx.py and export_bilateral_filter.py).  Conventions as in hiseg.h.
 *
 * Every entry point takes f32 NCHW planes with C folded into N: NC contiguous planes of H x W, x and out distinct
 * buffers of the same size (hiseg_opt_edge_smooth_fwd alone also takes f16 planes).  All arithmetic is f32.
 * NC * H * W == 0 returns HISEG_OK without a launch.
 *
 * Kernel forms (csrc/postprocess.hip).  A plane of at most 20480 pixels (two f32 working copies in the 160 KB of
 * LDS: the 64x48 and 128x96 instance masks) is owned by one workgroup: every iteration and stage runs LDS to LDS,
 * the plane is read once and written once.  Larger planes (the 480x640 binary masks) take 64x64 tiles with a
 * halo of iterations x radius pixels (summed radii for the morphological chain), at most 32; each tile recomputes
 * its halo, and pixels outside the image are re-padded as the reference pads them at every iteration.  Both forms
 * give the same bits, and N iterations in one launch the same bits as N launches.  force_tiled != 0 takes the
 * tiled form at any size (tests).
 */
#ifndef HISEG_POST_H_
#define HISEG_POST_H_

#include "hiseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host function (no GPU): the largest `iterations` one launch accepts for a stencil of this radius on H x W
 * planes -- 32 / radius in the tiled form, INT_MAX in the LDS-resident form.  A caller with more splits the
 * launches (the results are the same bits). */
int hiseg_post_max_iterations(int H, int W, int radius, int force_tiled);

/* BinaryMaskEdgeSmoothing.forward (edge_smoothing.py:34-90) applied `iterations` >= 1 times: 3x3 Laplacian,
 * e = sigmoid(|lap| * blur_strength), 3x3 (1,2,1)/16 Gaussian b, m*(1-e) + b*e, > threshold -> 1.0 / 0.0.  Both
 * convolutions zero padded.  The sigmoid and the blend are evaluated in f32 in the reference's operation order
 * (1/(1+exp(-x)), then m*(1-e) + b*e, no fused multiply-add): on a binary mask the reference's decision at a
 * blend of exactly 0.5 (sigmoid(18) rounds to 1.0f) is reproduced bit for bit.  binarize_input != 0 smooths the
 * mask (x > 0.5) instead of x (the probability-map path of MultiClassEdgeSmoothing, edge_smoothing.py:144). */
int hiseg_edge_smooth_fwd(const float* x, float* out, long long NC, int H, int W, float threshold,
                          float blur_strength, int iterations, int binarize_input, int force_tiled,
                          hiseg_stream_t stream);

/* MultiClassEdgeSmoothing.smooth_predictions, 3-class path (edge_smoothing.py:127-150): scores [B][3][H][W] ->
 * out [B][3][H][W], plane c = the mask (argmax over the 3 scores == c) smoothed `iterations` times as above.  On
 * ties the first maximum wins (torch.argmax); the one-hot planes are formed while loading and never reach
 * memory.  NaN scores are out of scope: a NaN is never the maximum here, while torch.argmax picks it. */
int hiseg_class_edge_smooth_fwd(const float* scores, float* out, long long B, int H, int W, float threshold,
                                float blur_strength, int iterations, int force_tiled, hiseg_stream_t stream);

/* BinaryMaskBilateralFilter.forward (bilateral_filter.py:349-406) and FastBilateralFilter.forward (158-216) in
 * one kernel.  Per iteration f = G*x, v = max(G*x^2 - f^2, 0), w = exp(-v * gain), x <- w*f + (1-w)*x, with G the
 * normalised kernel_size x kernel_size Gaussian of sigma_spatial (kernel_size odd, 3..9), zero padded.
 * gain: 10 for the binary-mask filter, 1 / (2 sigma_range^2) for the fast filter.  clamp_input != 0 clamps x to
 * [0, 1] first; threshold_output != 0 writes (x > threshold) as 1.0 / 0.0 instead of x. */
int hiseg_var_gated_blur_fwd(const float* x, float* out, long long NC, int H, int W, int kernel_size,
                             float sigma_spatial, float gain, int clamp_input, int threshold_output,
                             float threshold, int iterations, int force_tiled, hiseg_stream_t stream);

/* MorphologicalBilateralFilter.forward (bilateral_filter.py:473-501): clamp to [0, 1], open (min then max over
 * morph_size x morph_size), kernel_size x kernel_size normalised Gaussian of sigma (zero padded), close (max
 * then min), > 0.5 -> 1.0 / 0.0.  max_pool2d pads with -inf: neither min nor max sees the padding.  kernel_size
 * odd 3..9, morph_size odd 1..9. */
int hiseg_morph_bilateral_fwd(const float* x, float* out, long long NC, int H, int W, int kernel_size, float sigma,
                              int morph_size, int force_tiled, hiseg_stream_t stream);

/* BilateralFilter.forward (bilateral_filter.py:60-113): the true bilateral filter with reflect padding, weight
 * exp(-(dx^2+dy^2) / (2 sigma_spatial^2)) * exp(-(p - c)^2 / (2 sigma_range^2)), normalised by (sum + 1e-8).
 * H, W > kernel_size / 2 as F.pad(mode='reflect') requires, else HISEG_ERR_BAD_ARG. */
int hiseg_bilateral_fwd(const float* x, float* out, long long NC, int H, int W, int kernel_size,
                        float sigma_spatial, float sigma_range, hiseg_stream_t stream);

/* EdgePreservingFilter.forward (bilateral_filter.py:263-296), the guided filter: x [B][Cx][H][W], guide
 * [B][Cg][H][W] -> out [B][max(Cx, Cg)][H][W].  With box(t) the (2 radius + 1)^2 sum of t, zero padded and always
 * divided by (2 radius + 1)^2:
 *   a = (box(x*g) - box(x)*box(g)) / (box(g*g) - box(g)^2 + eps),  b = box(x) - a*box(g),  out = box(a)*g + box(b).
 * The variance is not clamped, and a and b are zero outside the image for the second pair of boxes, as the
 * reference's zero-padded convolutions have it.  guide == NULL: self-guided (g = x, Cg is ignored); guide may equal
 * x, out is distinct from both.  Channels broadcast as in x * guide: Cx == Cg or one of them is 1, else
 * HISEG_ERR_BAD_ARG; a plane that is broadcast is read once per output plane and never materialised.  radius 1..16.
 * Every box is a separable plain f32 sum (rows, then columns, taps in ascending order), independent of the tile.
 *
 * Forms.  The working set is six f32 planes (x, g, two planes of row sums, and box(x), box(g) that become a, b), so
 * a plane of at most 6826 pixels (160 KB / 24 B: the 64x48 instance masks; the 128x96 ones are tiled) is owned by
 * one workgroup and read from memory once.  Larger planes, or any with force_tiled != 0, take tiles 64 pixels wide
 * that recompute a and b on a halo of radius from inputs on a halo of 2 radius; the tile is 64 rows high up to
 * radius 6 and 32 / 16 / 8 rows up to radius 11 / 14 / 16, where 64 rows would not fit the LDS.  Both forms give the
 * same bits. */
int hiseg_guided_filter_fwd(const float* x, const float* guide, float* out, long long B, int Cx, int Cg, int H, int W,
                            int radius, float eps, int force_tiled, hiseg_stream_t stream);

/* ---- The other three edge-smoothing graphs of export_edge_smoothing_onnx.py.  All three are stencils of radius 2
 * (hiseg_post_max_iterations(H, W, 2, force_tiled): 16 iterations per launch in the tiled form), applied
 * `iterations` >= 1 times, every convolution zero padded, the blend m*(1-e) + b*e evaluated as in
 * hiseg_edge_smooth_fwd (each operation rounded to f32 on its own, no fused multiply-add).  x, out and soft are
 * distinct buffers of NC planes.  soft, when not NULL, receives the f32 blend of the LAST iteration before its
 * threshold (out is the decision soft > threshold); each element of out and of soft is written by one thread.
 * Both kernel forms give the same bits, and N iterations in one launch the same bits as N launches. */

/* DirectionalEdgeSmoothing.forward (:114-155): Sobel ex, ey; mag = sqrt(ex^2 + ey^2 + 1e-8), t = atan2(ey, ex); the
 * blurs 1x5 and 5x1 (0.1, 0.2, 0.4, 0.2, 0.1) and the two 3x3 diagonals (0.1, 0.8, 0.1); weights cos^2 t, sin^2 t,
 * 0.5 cos^2(t - pi/4), 0.5 cos^2(t + pi/4), each divided by (their sum + 1e-8); e = sigmoid(3 mag); > 0.5.  The
 * f32 libm functions and the divisions are the IEEE ones, not the fast intrinsics. */
int hiseg_dir_edge_smooth_fwd(const float* x, float* out, float* soft, long long NC, int H, int W, int iterations,
                              int force_tiled, hiseg_stream_t stream);

/* AdaptiveEdgeSmoothing.forward (:172-213): e = (|3x3 Laplacian| > 0.5 edge_sensitivity) as 0 / 1, a = 5x5 mean,
 * s = m*(1 - bs/3) + a*(bs/3), m*(1-e) + s*e, > final_threshold.  The three parameters are DEVICE arrays read by the
 * kernel, never by the host: plane p uses element p * param_stride of each, so param_stride 0 broadcasts element 0
 * to every plane and 1 gives every plane its own (NC elements). */
int hiseg_adaptive_edge_smooth_fwd(const float* x, float* out, float* soft, long long NC, int H, int W,
                                   const float* blur_strength, const float* edge_sensitivity,
                                   const float* final_threshold, long long param_stride, int iterations,
                                   int force_tiled, hiseg_stream_t stream);

/* OptimizedEdgeSmoothing.forward (:279-318): 3x3 Laplacian, the separable (1, 4, 6, 4, 1)/16 Gaussian (horizontal
 * sums first, then the vertical sum of those), e = clamp((3 |lap| + 0.5) * 0.5, 0, 1), the blend, > 0.5.  dtype is
 * the type of the planes x and out: HISEG_POST_F32 (use_fp16=False), HISEG_POST_F16 (use_fp16=True), or
 * HISEG_POST_F32_TO_F16 (use_fp16=True on an f32 mask: x is f32 and rounded to f16, to nearest even, while it is
 * read; out is f16; the same bits as casting x first), else HISEG_ERR_BAD_DTYPE.  With f16 planes the arithmetic is
 * f32 on the f16 values read, and the 0 / 1 written is exact in f16; soft is f32 either way. */
enum hiseg_post_dtype { HISEG_POST_F32 = 0, HISEG_POST_F16 = 2, HISEG_POST_F32_TO_F16 = 3 };
int hiseg_opt_edge_smooth_fwd(int dtype, const void* x, void* out, float* soft, long long NC, int H, int W,
                              int iterations, int force_tiled, hiseg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
