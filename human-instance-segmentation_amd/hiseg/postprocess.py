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
           "FastBilateralFilter", "EdgePreservingFilter", "BinaryMaskBilateralFilter", "MorphologicalBilateralFilter"]


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
