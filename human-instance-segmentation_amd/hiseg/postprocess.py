"""Mask post-processing: the reference's edge-smoothing and bilateral-filter modules on libhiseg
(include/hiseg_post.h, csrc/postprocess.hip).

Class names, constructor arguments, defaults and registered buffers follow
src/human_edge_detection/edge_smoothing.py and bilateral_filter.py, so ``state_dict()`` keys and shapes are the
reference's.  The buffers are built once in ``__init__`` as the reference builds them and exist for that
compatibility: every forward is one fused HIP kernel that derives its weights from the constructor arguments
(``kernel_size``, ``sigma*``), not from the buffers.  There is no torch arithmetic in any forward and no CPU
path: a CPU tensor raises ``RuntimeError``.

Differences from the reference, all on inputs it mishandles or leaves to chance:
  * ``MorphologicalBilateralFilter`` works on any channel count (the reference's conv weight fixes C = 1) and
    refuses even ``kernel_size`` / ``morph_size`` (the reference returns a plane of another size);
  * ``kernel_size`` is limited to 3..9 (``morph_size`` 1..9), the ``radius`` of ``EdgePreservingFilter`` to 1..16;
  * ``MultiClassEdgeSmoothing.smooth_predictions(apply_softmax=True)``: with 3 classes the softmax is skipped, as
    the argmax of the scores is the argmax of their softmax; with another class count it is not implemented;
  * NaN scores in the 3-class path are out of scope (hiseg_post.h).
"""
from __future__ import annotations

from typing import Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import ops

__all__ = ["BinaryMaskEdgeSmoothing", "MultiClassEdgeSmoothing", "apply_edge_smoothing_to_masks", "BilateralFilter",
           "FastBilateralFilter", "EdgePreservingFilter", "BinaryMaskBilateralFilter", "MorphologicalBilateralFilter",
           "DirectionalEdgeSmoothing", "AdaptiveEdgeSmoothing", "OptimizedEdgeSmoothing"]


def _check_kernel_size(kernel_size: int, what: str = "Kernel size", lo: int = 3) -> None:
    if kernel_size % 2 == 0:
        raise ValueError(f"{what} must be odd")
    if not lo <= kernel_size <= 9:
        raise ValueError(f"{what} must be in {lo}..9, got {kernel_size}")


def _centred_coords(kernel_size: int) -> torch.Tensor:
    coords = torch.arange(kernel_size, dtype=torch.float32)
    return coords - (kernel_size - 1) / 2


def _gaussian_1d(kernel_size: int, sigma: float) -> torch.Tensor:
    k = torch.exp(-_centred_coords(kernel_size) ** 2 / (2 * sigma ** 2))
    return k / k.sum()


def _gaussian_2d_unnormalised(kernel_size: int, sigma: float) -> torch.Tensor:
    c = _centred_coords(kernel_size)
    y = c.view(-1, 1).expand(kernel_size, kernel_size)
    x = c.view(1, -1).expand(kernel_size, kernel_size)
    return torch.exp(-(x ** 2 + y ** 2) / (2 * sigma ** 2))


def _nchw(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() != 4:
        raise ValueError(f"{what}: expected a (B, C, H, W) tensor, got shape {tuple(x.shape)}")
    return x


class BinaryMaskEdgeSmoothing(nn.Module):
    """Edge smoothing of binary masks (edge_smoothing.py:10-90): (B, C, H, W), (C, H, W) or (H, W) in, the same
    shape and dtype out."""

    def __init__(self, threshold: float = 0.5, blur_strength: float = 3.0):
        super().__init__()
        self.threshold = threshold
        self.blur_strength = blur_strength
        self.register_buffer("laplacian_kernel", torch.tensor(
            [[-1, -1, -1], [-1, 8, -1], [-1, -1, -1]], dtype=torch.float32).unsqueeze(0).unsqueeze(0))
        self.register_buffer("gaussian_kernel", torch.tensor(
            [[1 / 16, 2 / 16, 1 / 16], [2 / 16, 4 / 16, 2 / 16], [1 / 16, 2 / 16, 1 / 16]],
            dtype=torch.float32).unsqueeze(0).unsqueeze(0))

    def forward(self, mask: torch.Tensor, iterations: int = 1) -> torch.Tensor:
        if mask.dim() not in (2, 3, 4):
            raise ValueError(f"expected a (B, C, H, W), (C, H, W) or (H, W) mask, got shape {tuple(mask.shape)}")
        return ops.edge_smooth(mask, self.threshold, self.blur_strength, iterations).to(mask.dtype)


class MultiClassEdgeSmoothing:
    """Multi-class segmentation mask edge smoothing (edge_smoothing.py:93-170)."""

    def __init__(self, threshold: float = 0.5, blur_strength: float = 3.0, iterations: int = 1,
                 device: str = "cuda"):
        self.smoother = BinaryMaskEdgeSmoothing(threshold, blur_strength)
        self.smoother.to(device)
        self.smoother.eval()
        self.iterations = iterations
        self.device = device

    def smooth_predictions(self, predictions: Union[torch.Tensor, np.ndarray],
                           apply_softmax: bool = False) -> Union[torch.Tensor, np.ndarray]:
        """(B, C, H, W) or (C, H, W) predictions -> one smoothed 0/1 mask per class: argmax == c for 3 classes,
        predictions[:, c] > 0.5 otherwise.  A batch of one is squeezed; numpy in, numpy out."""
        is_numpy = isinstance(predictions, np.ndarray)
        if is_numpy:
            predictions = torch.from_numpy(predictions)
        predictions = predictions.to(self.device)
        if predictions.dim() == 3:
            predictions = predictions.unsqueeze(0)
        if predictions.dim() != 4:
            raise ValueError(f"expected (B, C, H, W) or (C, H, W) predictions, got shape {tuple(predictions.shape)}")
        s = self.smoother
        with torch.no_grad():
            if predictions.shape[1] == 3:
                smoothed = ops.class_edge_smooth(predictions, s.threshold, s.blur_strength, self.iterations)
            elif apply_softmax:
                raise NotImplementedError("apply_softmax with a class count other than 3: pass probabilities")
            else:
                smoothed = ops.edge_smooth(predictions, s.threshold, s.blur_strength, self.iterations,
                                           binarize_input=True)
        if smoothed.shape[0] == 1:
            smoothed = smoothed.squeeze(0)
        return smoothed.cpu().numpy() if is_numpy else smoothed


def apply_edge_smoothing_to_masks(masks: Union[torch.Tensor, np.ndarray], threshold: float = 0.5,
                                  blur_strength: float = 3.0, iterations: int = 1,
                                  device: str = "cuda") -> Union[torch.Tensor, np.ndarray]:
    """Convenience wrapper (edge_smoothing.py:173-192)."""
    return MultiClassEdgeSmoothing(threshold, blur_strength, iterations, device).smooth_predictions(masks)


class BilateralFilter(nn.Module):
    """The true bilateral filter with reflect padding (bilateral_filter.py:9-113)."""

    def __init__(self, kernel_size: int = 5, sigma_spatial: float = 1.0, sigma_range: float = 0.1):
        super().__init__()
        _check_kernel_size(kernel_size)
        self.kernel_size = kernel_size
        self.sigma_spatial = sigma_spatial
        self.sigma_range = sigma_range
        self.padding = kernel_size // 2
        self.register_buffer("spatial_kernel", _gaussian_2d_unnormalised(kernel_size, sigma_spatial))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _nchw(x, "BilateralFilter")
        return ops.bilateral(x, self.kernel_size, self.sigma_spatial, self.sigma_range)


class FastBilateralFilter(nn.Module):
    """Variance-gated separable Gaussian (bilateral_filter.py:116-216)."""

    def __init__(self, kernel_size: int = 5, sigma_spatial: float = 1.0, sigma_range: float = 0.1,
                 num_iterations: int = 2):
        super().__init__()
        _check_kernel_size(kernel_size)
        self.kernel_size = kernel_size
        self.sigma_spatial = sigma_spatial
        self.sigma_range = sigma_range
        self.num_iterations = num_iterations
        self.padding = kernel_size // 2
        kernel_1d = _gaussian_1d(kernel_size, sigma_spatial)
        self.register_buffer("kernel_h", kernel_1d.view(1, 1, 1, kernel_size))
        self.register_buffer("kernel_v", kernel_1d.view(1, 1, kernel_size, 1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _nchw(x, "FastBilateralFilter")
        if self.num_iterations < 1:
            ops._require_gpu(x)
            return x
        return ops.var_gated_blur(x, self.kernel_size, self.sigma_spatial, 1.0 / (2 * self.sigma_range ** 2),
                                  self.num_iterations)


class EdgePreservingFilter(nn.Module):
    """Guided filter (bilateral_filter.py:219-296): x smoothed where ``guide`` (default: x itself) is flat, kept
    where it has edges.  (B, C, H, W) or (C, H, W) in; the channels of x and guide broadcast as in ``x * guide``."""

    def __init__(self, radius: int = 2, eps: float = 0.01):
        super().__init__()
        if not 1 <= radius <= 16:
            raise ValueError(f"radius must be in 1..16, got {radius}")
        self.radius = radius
        self.eps = eps
        self.kernel_size = 2 * radius + 1
        kernel = torch.ones(1, 1, self.kernel_size, self.kernel_size)
        self.register_buffer("box_kernel", kernel / (self.kernel_size ** 2))

    def forward(self, x: torch.Tensor, guide: Optional[torch.Tensor] = None) -> torch.Tensor:
        if x.dim() not in (3, 4) or (guide is not None and guide.dim() != x.dim()):
            raise ValueError("EdgePreservingFilter: expected (B, C, H, W) or (C, H, W) tensors of one rank, got "
                             f"{tuple(x.shape)}" + ("" if guide is None else f" and {tuple(guide.shape)}"))
        if x.dim() == 3:
            return ops.guided_filter(x.unsqueeze(0), None if guide is None else guide.unsqueeze(0), self.radius,
                                     self.eps).squeeze(0)
        return ops.guided_filter(x, guide, self.radius, self.eps)


class BinaryMaskBilateralFilter(nn.Module):
    """Variance-gated Gaussian for binary masks, thresholded (bilateral_filter.py:299-406)."""

    def __init__(self, kernel_size: int = 7, sigma_spatial: float = 1.5, threshold: float = 0.5,
                 num_iterations: int = 2):
        super().__init__()
        _check_kernel_size(kernel_size)
        self.kernel_size = kernel_size
        self.sigma_spatial = sigma_spatial
        self.threshold = threshold
        self.num_iterations = num_iterations
        self.padding = kernel_size // 2
        g = _gaussian_2d_unnormalised(kernel_size, sigma_spatial)
        self.register_buffer("gaussian_kernel", (g / g.sum()).view(1, 1, kernel_size, kernel_size))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _nchw(x, "BinaryMaskBilateralFilter")
        if self.num_iterations < 1:
            raise ValueError("num_iterations must be >= 1")
        return ops.var_gated_blur(x, self.kernel_size, self.sigma_spatial, 10.0, self.num_iterations,
                                  clamp_input=True, threshold=self.threshold)


class MorphologicalBilateralFilter(nn.Module):
    """Open, Gaussian, close, threshold (bilateral_filter.py:409-501)."""

    def __init__(self, kernel_size: int = 5, sigma: float = 1.0, morph_size: int = 3):
        super().__init__()
        _check_kernel_size(kernel_size)
        _check_kernel_size(morph_size, "Morphological size", lo=1)
        self.kernel_size = kernel_size
        self.sigma = sigma
        self.morph_size = morph_size
        self.padding = kernel_size // 2
        self.morph_padding = morph_size // 2
        kernel_1d = _gaussian_1d(kernel_size, sigma)
        self.register_buffer("bilateral_kernel",
                             (kernel_1d.view(-1, 1) * kernel_1d.view(1, -1)).view(1, 1, kernel_size, kernel_size))
        self.register_buffer("morph_kernel", torch.ones(1, 1, morph_size, morph_size))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _nchw(x, "MorphologicalBilateralFilter")
        return ops.morph_bilateral(x, self.kernel_size, self.sigma, self.morph_size)


# ---- the directional, adaptive and optimized graphs of export_edge_smoothing_onnx.py
#
# The registered buffers (and the three frozen convolutions of OptimizedEdgeSmoothing) carry the reference's
# state_dict keys and values so that its checkpoints load strictly.  The kernels use those taps as constants: a
# loaded value that differs from the reference's raises, instead of being ignored.


def _kernel4(rows) -> torch.Tensor:
    return torch.tensor(rows, dtype=torch.float32).unsqueeze(0).unsqueeze(0)


_LAPLACIAN = [[-1, -1, -1], [-1, 8, -1], [-1, -1, -1]]
_GAUSS5 = [0.0625, 0.25, 0.375, 0.25, 0.0625]


class _FixedTaps(nn.Module):
    """A module whose state is constant: remembers it at construction and checks every load against it."""

    def _freeze_taps(self) -> None:
        self._taps = {k: v.detach().clone() for k, v in self.state_dict().items()}
        self.register_load_state_dict_post_hook(_FixedTaps._check_taps)

    @staticmethod
    def _check_taps(module, incompatible_keys) -> None:
        for k, v in module.state_dict().items():
            want = module._taps[k]
            if v.shape != want.shape or not torch.equal(v.detach().float().cpu(), want):
                raise ValueError(f"{type(module).__name__}: loaded '{k}' differs from the reference's constant; the "
                                 "kernel computes with the fixed taps")

    @staticmethod
    def _mask(mask: torch.Tensor, what: str, dtypes=(torch.float32,)) -> torch.Tensor:
        if not isinstance(mask, torch.Tensor) or mask.dim() != 4:
            raise ValueError(f"{what}: expected a (B, C, H, W) mask, got "
                             f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}")
        if mask.dtype not in dtypes:
            raise ValueError(f"{what}: expected a mask of {' or '.join(str(d) for d in dtypes)}, got {mask.dtype}")
        return mask


class DirectionalEdgeSmoothing(_FixedTaps):
    """Direction-aware edge smoothing (export_edge_smoothing_onnx.py:63-155): (B, C, H, W) float32 in, 0/1 float32
    out.  ``num_directions`` is stored and never read, as in the reference."""

    def __init__(self, num_directions: int = 4):
        super().__init__()
        self.num_directions = num_directions
        self.register_buffer("sobel_x", _kernel4([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]))
        self.register_buffer("sobel_y", _kernel4([[-1, -2, -1], [0, 0, 0], [1, 2, 1]]))
        self.register_buffer("h_blur", _kernel4([[0.1, 0.2, 0.4, 0.2, 0.1]]))
        self.register_buffer("v_blur", _kernel4([[0.1], [0.2], [0.4], [0.2], [0.1]]))
        self.register_buffer("diag1_blur", _kernel4([[0.1, 0.0, 0.0], [0.0, 0.8, 0.0], [0.0, 0.0, 0.1]]))
        self.register_buffer("diag2_blur", _kernel4([[0.0, 0.0, 0.1], [0.0, 0.8, 0.0], [0.1, 0.0, 0.0]]))
        self._freeze_taps()

    def forward(self, mask: torch.Tensor, iterations: int = 1, return_soft: bool = False):
        self._mask(mask, "DirectionalEdgeSmoothing")
        return ops.dir_edge_smooth(mask, iterations, return_soft=return_soft)


class AdaptiveEdgeSmoothing(_FixedTaps):
    """Edge smoothing with run-time parameters (export_edge_smoothing_onnx.py:158-213): ``forward(mask,
    blur_strength, edge_sensitivity, final_threshold)`` with (B, 1) float32 tensors on the mask's device (one value
    per image; one element broadcasts).  The kernel reads them on the device: no host synchronisation, and a
    captured graph sees the values they hold at replay.

    The three parameters may also be given at construction, as floats or tensors; they are then kept on the
    module's device and ``forward(mask)`` is a callable of one tensor (a serving hook)."""

    def __init__(self, blur_strength=None, edge_sensitivity=None, final_threshold=None):
        super().__init__()
        self.register_buffer("laplacian_kernel", _kernel4(_LAPLACIAN))
        self._freeze_taps()
        for name, v in (("blur_strength", blur_strength), ("edge_sensitivity", edge_sensitivity),
                        ("final_threshold", final_threshold)):
            if v is not None and not isinstance(v, torch.Tensor):
                v = torch.tensor([float(v)], dtype=torch.float32)
            if v is not None and v.dtype != torch.float32:
                raise ValueError(f"AdaptiveEdgeSmoothing: {name} must be a float or a float32 tensor, got {v.dtype}")
            self.register_buffer("default_" + name, v, persistent=False)

    def forward(self, mask: torch.Tensor, blur_strength: Optional[torch.Tensor] = None,
                edge_sensitivity: Optional[torch.Tensor] = None, final_threshold: Optional[torch.Tensor] = None,
                iterations: int = 1, return_soft: bool = False):
        self._mask(mask, "AdaptiveEdgeSmoothing")
        params = []
        for name, v in (("blur_strength", blur_strength), ("edge_sensitivity", edge_sensitivity),
                        ("final_threshold", final_threshold)):
            v = getattr(self, "default_" + name) if v is None else v
            if v is None:
                raise ValueError(f"AdaptiveEdgeSmoothing: {name} was given neither to forward nor at construction")
            params.append(v)
        return ops.adaptive_edge_smooth(mask, *params, iterations, return_soft=return_soft)


class OptimizedEdgeSmoothing(_FixedTaps):
    """The deployment variant (export_edge_smoothing_onnx.py:216-318): Laplacian, separable 5-tap Gaussian and a
    clamped linear ramp in place of the sigmoid.  ``use_fp16=True``: a float32 mask is rounded to float16 as the
    reference does -- by the kernel while it reads the mask, not by a cast pass -- a float16 mask is taken as it
    is, and the 0/1 result is float16 (float32 arithmetic on the float16 values).
    ``use_fp16=False``: float32 in and out.  The three convolutions exist for the reference's state_dict keys and
    are never called."""

    def __init__(self, use_fp16: bool = True):
        super().__init__()
        self.use_fp16 = use_fp16
        self.edge_detector = nn.Conv2d(1, 1, kernel_size=3, padding=1, groups=1, bias=False)
        self.gaussian_h = nn.Conv2d(1, 1, kernel_size=(1, 5), padding=(0, 2), bias=False)
        self.gaussian_v = nn.Conv2d(1, 1, kernel_size=(5, 1), padding=(2, 0), bias=False)
        for conv, taps, shape in ((self.edge_detector, _LAPLACIAN, (1, 1, 3, 3)), (self.gaussian_h, _GAUSS5, (1, 1, 1, 5)),
                                  (self.gaussian_v, _GAUSS5, (1, 1, 5, 1))):
            conv.weight.data = torch.tensor(taps, dtype=torch.float32).reshape(shape)
            conv.weight.requires_grad = False
        self.register_buffer("edge_scale", torch.tensor(3.0))
        self.register_buffer("threshold", torch.tensor(0.5))
        self._freeze_taps()

    def forward(self, mask: torch.Tensor, iterations: int = 1, return_soft: bool = False):
        if self.use_fp16:
            self._mask(mask, "OptimizedEdgeSmoothing", (torch.float32, torch.float16))
        else:
            self._mask(mask, "OptimizedEdgeSmoothing(use_fp16=False)")
        return ops.opt_edge_smooth(mask, iterations, to_fp16=self.use_fp16, return_soft=return_soft)
