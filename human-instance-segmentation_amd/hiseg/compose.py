"""Full-frame instance composition: per-ROI masks -> one label map and one colour overlay per frame, on libhiseg
(include/hiseg_compose.h, csrc/compose.hip).

This is the consumer stage of the reference's serving script (test_hierarchical_instance_peopleseg_onnx.py):
``process_mask_output`` (:230-291) thresholds each ROI's softmax, scores it and resizes its mask to its pixel box
with cv2's nearest map; ``visualize_instance_segmentation`` (:336-402) pastes the masks into the frame, the later
ROI repainting the earlier, and blends the colours with the image.  Here the three steps are three kernels and the
label map -- which ROI owns each pixel -- is a result of its own.

Differences from the reference:
  * a box that reaches outside the frame is clipped to it, with the mask still mapped over the unclipped box; the
    reference raises there (its slice assignment does not broadcast);
  * the reference counts colours over the ROIs one frame keeps (it drops the boxes that are empty in pixels before
    it numbers them); ``overlay`` takes a colour per row of ``rois``, so a caller who wants the reference's picture
    passes a table built that way, and the default is ``instance_colors(N)`` over all rows;
  * NaN logits are out of scope (hiseg_compose.h).

There is no torch arithmetic in any call, no host synchronisation and no CPU path: a CPU tensor raises
``RuntimeError``, and every call can sit inside a captured graph.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import ops

__all__ = ["InstanceMapComposer", "instance_colors"]

# matplotlib's 'hsv' colormap (matplotlib/_cm.py _hsv_data): piecewise-linear segments (x, y) per channel
_HSV_SEGMENTS = {
    "red": ((0.0, 1.0), (0.15873, 1.0), (0.174603, 0.96875), (0.333333, 0.03125), (0.349206, 0.0), (0.666667, 0.0),
            (0.68254, 0.03125), (0.84127, 0.96875), (0.857143, 1.0), (1.0, 1.0)),
    "green": ((0.0, 0.0), (0.15873, 0.9375), (0.174603, 1.0), (0.507937, 1.0), (0.666667, 0.0625), (0.68254, 0.0),
              (1.0, 0.0)),
    "blue": ((0.0, 0.0), (0.333333, 0.0), (0.349206, 0.0625), (0.507937, 1.0), (0.84127, 1.0), (0.857143, 0.9375),
             (1.0, 0.09375)),
}
_HSV_LUT = None


def _hsv_lut() -> np.ndarray:
    """The colormap's 256-entry lookup table [256, 3], float64, with the arithmetic of matplotlib's
    LinearSegmentedColormap (colors._create_lookup_table, gamma 1) in its operation order."""
    global _HSV_LUT
    if _HSV_LUT is None:
        n = 256
        chans = []
        for name in ("red", "green", "blue"):
            seg = np.array(_HSV_SEGMENTS[name])
            x, y = seg[:, 0] * (n - 1), seg[:, 1]
            xind = (n - 1) * np.linspace(0, 1, n) ** 1.0
            ind = np.searchsorted(x, xind)[1:-1]
            distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
            lut = np.concatenate([[y[0]], distance * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
            chans.append(np.clip(lut, 0.0, 1.0))
        _HSV_LUT = np.stack(chans, axis=1)
    return _HSV_LUT


def instance_colors(n: int) -> torch.Tensor:
    """generate_instance_colors (:106-115) as a uint8 tensor [n, 3] on the host: hues ``linspace(0, 1, n + 1)[:-1]``
    through matplotlib's ``hsv`` colormap (entry ``int(hue * 256)`` of its 256-entry table), ``int(c * 255)`` per
    channel.  matplotlib is not imported; the table is restated from the colormap's segments."""
    n = int(n)
    if n < 0:
        raise ValueError(f"instance_colors: n = {n}")
    hues = np.linspace(0, 1, n + 1)[:-1]
    idx = np.clip((hues * 256).astype(np.int64), 0, 255)
    rgb = _hsv_lut()[idx]
    return torch.from_numpy((rgb * 255).astype(np.int64).astype(np.uint8).reshape(n, 3))


class InstanceMapComposer(nn.Module):
    """Per-ROI masks or logits -> the frame's label map.

    ``forward(masks_or_logits, rois, frame_size=None)`` returns ``(label, score)``: ``label`` int32 [B,H,W] with 0 for
    background and k + 1 where ROI k (row k of ``rois`` [N,5]: batch index, x1, y1, x2, y2 normalised) owns the pixel;
    ``score`` f32 [N].  With ``from_logits`` the input is the model's logits [N,3,mh,mw] and a pixel belongs to the
    target when the argmax is class 1 and the softmax maximum exceeds ``score_threshold``; ``score`` is the mean of
    that maximum over the target pixels.  Without it the input is the exported contract's ``instance_masks``
    [N,1,mh,mw] (set where > 0.5; ``score`` is 1 for a ROI with a target pixel, else 0).  ROIs with ``score <= 0`` or
    a box that is empty in pixels own nothing.

    ``frame_size`` is (B, H, W), the frames the boxes are scaled to -- the original images, which need not have the
    model's input size.  The number of frames cannot be read from ``rois`` without a host synchronisation, so it is
    always given; a composer built with ``frame_size=(H, W)`` takes the batch from the call's ``frame_size=(B,)`` or
    (B, H, W).

    ``overlay(label, image, colors=None, alpha=0.5)`` blends uint8 frames [B,H,W,3] with the owners' colours
    (``colors`` uint8 [N,3] or the ROI count; default ``instance_colors(N)`` for the N of the latest forward, uploaded
    once per count and device -- so warm it up before capturing a graph) as cv2.addWeighted does.
    """

    def __init__(self, frame_size=None, score_threshold: float = 0.5, from_logits: bool = True):
        super().__init__()
        if frame_size is not None:
            frame_size = tuple(int(v) for v in frame_size)
            if len(frame_size) not in (2, 3):
                raise ValueError(f"frame_size must be (H, W) or (B, H, W), got {frame_size}")
        self.frame_size = frame_size
        self.score_threshold = float(score_threshold)
        self.from_logits = bool(from_logits)
        self._colors = {}
        self._last_n = None

    def resolve_frame_size(self, frame_size=None, batch=None):
        """(B, H, W) from the call's ``frame_size`` ((B, H, W), (H, W) or (B,)), the composer's own and ``batch``."""
        own = self.frame_size or ()
        fs = tuple(int(v) for v in frame_size) if frame_size is not None else ()
        if len(fs) == 3:
            return fs
        if len(fs) == 1:
            batch, fs = fs[0], ()
        hw = fs if len(fs) == 2 else own[-2:]
        if batch is None and len(own) == 3:
            batch = own[0]
        if len(hw) != 2 or batch is None:
            raise ValueError("InstanceMapComposer: the frame size (B, H, W) is not known: pass frame_size=(B, H, W) "
                             "(the batch size cannot be read from rois without a host synchronisation)")
        return (int(batch), int(hw[0]), int(hw[1]))

    def pack(self, masks_or_logits: torch.Tensor):
        """(bits, score, count) of the configured front end."""
        if self.from_logits:
            return ops.roi_mask_classify(masks_or_logits, self.score_threshold)
        return ops.roi_mask_pack(masks_or_logits)

    def forward(self, masks_or_logits: torch.Tensor, rois: torch.Tensor, frame_size=None):
        fs = self.resolve_frame_size(frame_size)
        bits, score, _ = self.pack(masks_or_logits)
        self._last_n = int(rois.shape[0])
        label = ops.compose_instance_map(bits, score, rois, fs, masks_or_logits.shape[-1])
        return label, score

    def overlay(self, label: torch.Tensor, image: torch.Tensor, colors=None, alpha: float = 0.5):
        if colors is None:              # the ROI count of the latest forward (a label map does not carry it)
            if self._last_n is None:
                raise ValueError("InstanceMapComposer.overlay: colors=None needs the ROI count of a forward of this "
                                 "composer; pass colors (uint8 [N,3]) or the count")
            colors = self._last_n
        if isinstance(colors, int):     # the default table for that many ROIs, uploaded once per (n, device)
            key = (colors, str(label.device))
            if key not in self._colors:
                self._colors[key] = instance_colors(colors).to(label.device)
            colors = self._colors[key]
        return ops.instance_overlay(label, image, colors, alpha)
