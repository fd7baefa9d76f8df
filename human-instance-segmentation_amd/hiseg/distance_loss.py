"""DistanceAwareSegmentationLoss, AdaptiveBoundaryLoss and create_distance_aware_loss on libhiseg
(advanced/distance_aware_loss.py:188-437 over losses.py:9-127, :204-277).

Same constructors, the same call ``loss_fn(predictions, targets, instance_info=None) -> (total, loss_dict)`` and the
same loss-dict keys as the reference.  The reference builds the boundary weight map per ROI on the host (numpy,
scipy's distance_transform_edt, a copy back); here the exact Euclidean distance transform, the weight map, the loss
and its backward are HIP kernels (include/hiseg_distance.h), so a step makes no host synchronisation and can be
captured in a graph.  ``loss_dict`` is lazy: one device->host copy on first access.  The quirks of the reference
that are reproduced are listed in DESIGN.md §4 "Distance-aware loss".
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .losses import LazyLossDict

_KEYS = ("total_loss", "ce_loss", "dice_loss", "boundary_accuracy", "avg_boundary_weight")
NOUT = 8   # include/hiseg_distance.h HISEG_DISTANCE_NOUT


class LazyDistanceLossDict(LazyLossDict):
    """dict[str, float] view of the distance-aware loss outputs (and, under AdaptiveBoundaryLoss, the two adaptive
    parameters appended to them); one device->host copy on first access."""

    def __init__(self, out: torch.Tensor, extra_keys: Sequence[str] = ()):
        super().__init__(out, list(_KEYS) + list(extra_keys), {})

    def _materialise(self, host=None) -> Dict[str, float]:
        if self._vals is None:
            if host is None:
                host = self._out.detach().cpu().tolist()
            v = {k: host[i] for i, k in enumerate(_KEYS)}
            for i, k in enumerate(self._keys[len(_KEYS):]):
                v[k] = host[NOUT + i]
            self._vals = v
        return self._vals


class _DistanceLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, handle, pred, target):
        lib = L.lib()
        N, _, H, W = pred.shape
        dev = pred.device
        weights, d2 = ops.boundary_weight_map(
            target, handle["width"], handle["boundary_weight"], handle["instance_sep_weight"], handle["inst"],
            handle["present"], dev_weights=handle["dev_weights"], force_tiled=handle["force_tiled"])
        ws = torch.empty(int(lib.hiseg_distance_ws(N, H, W)), dtype=torch.float32, device=dev)
        out = torch.empty(NOUT, dtype=torch.float32, device=dev)
        cw = handle["class_weights"]
        L.check(lib.hiseg_distance_loss_fwd(pred.data_ptr(), target.data_ptr(), weights.data_ptr(), N, H, W,
                                            cw.data_ptr() if cw is not None else None, int(handle["use_focal"]),
                                            float(handle["focal_gamma"]), float(handle["ce_weight"]),
                                            float(handle["dice_weight"]), ws.data_ptr(), out.data_ptr(),
                                            L.stream_ptr()), "distance_loss_fwd")
        ctx.save_for_backward(pred, target, weights, ws)
        ctx.cw, ctx.use_focal, ctx.gamma = cw, int(handle["use_focal"]), float(handle["focal_gamma"])
        ctx.mark_non_differentiable(out)
        handle["weights"], handle["d2"] = weights, d2
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g_total, _g_out):
        pred, target, weights, ws = ctx.saved_tensors
        N, _, H, W = pred.shape
        dp = torch.empty_like(pred)
        g = g_total.contiguous().float()
        cw = ctx.cw
        L.check(L.lib().hiseg_distance_loss_bwd(pred.data_ptr(), target.data_ptr(), weights.data_ptr(), N, H, W,
                                                cw.data_ptr() if cw is not None else None, ctx.use_focal, ctx.gamma,
                                                ws.data_ptr(), g.data_ptr(), dp.data_ptr(), L.stream_ptr()),
                "distance_loss_bwd")
        return None, dp, None


class _WeightGenerator:
    """The reference's BoundaryWeightGenerator as a parameter holder (distance_aware_loss.py:127-145); the map
    itself is hiseg.ops.boundary_weight_map."""

    def __init__(self, boundary_width: int = 5, boundary_weight: float = 2.0, instance_sep_weight: float = 3.0):
        self.boundary_width = boundary_width
        self.boundary_weight = boundary_weight
        self.instance_sep_weight = instance_sep_weight


InstanceInfo = Union[None, torch.Tensor, List[Optional[dict]]]


def _instance_maps(instance_info: InstanceInfo, N: int, H: int, W: int, dev):
    """(inst f32 [N,H,W] on dev, present uint8 [N] on dev) or (None, None).  ``instance_info``: None, a tensor
    [N,H,W], or the reference's list of per-sample dicts ('instance_distances' optional per dict).  CPU maps are
    stacked on the host and uploaded in one copy."""
    if instance_info is None:
        return None, None
    if isinstance(instance_info, torch.Tensor):
        if tuple(instance_info.shape) != (N, H, W):
            raise ValueError(f"instance_info: expected [{N},{H},{W}], got {tuple(instance_info.shape)}")
        return (instance_info.to(device=dev, dtype=torch.float32).contiguous(),
                torch.ones(N, dtype=torch.uint8, device=dev))
    if len(instance_info) == 0:   # `if instance_info` is false for an empty list (distance_aware_loss.py:269)
        return None, None
    if len(instance_info) != N:
        raise ValueError(f"instance_info: {len(instance_info)} entries for {N} samples")
    maps = [d.get("instance_distances") if d else None for d in instance_info]
    if all(m is None for m in maps):
        return None, None
    for m in maps:
        if m is not None and tuple(m.shape) != (H, W):
            raise ValueError(f"instance_distances: expected [{H},{W}], got {tuple(m.shape)}")
    present = torch.tensor([m is not None for m in maps], dtype=torch.uint8)
    if all(m is None or not m.is_cuda for m in maps):
        host = torch.stack([torch.zeros(H, W) if m is None else m.detach().to(torch.float32) for m in maps])
        return host.to(dev, non_blocking=True), present.to(dev, non_blocking=True)
    zero = torch.zeros(H, W, dtype=torch.float32, device=dev)
    inst = torch.stack([zero if m is None else m.detach().to(device=dev, dtype=torch.float32) for m in maps])
    return inst, present.to(dev, non_blocking=True)


class DistanceAwareSegmentationLoss(nn.Module):
    """Boundary-weighted CE (or focal) + class-1 Dice (distance_aware_loss.py:188-310); arguments as the reference."""

    def __init__(self, class_weights: Optional[torch.Tensor] = None, ce_weight: float = 1.0,
                 dice_weight: float = 1.0, boundary_width: int = 5, boundary_weight: float = 2.0,
                 instance_sep_weight: float = 3.0, use_focal: bool = False, focal_gamma: float = 2.0):
        super().__init__()
        self.class_weights = class_weights
        self.ce_weight = ce_weight
        self.dice_weight = dice_weight
        self.weight_generator = _WeightGenerator(boundary_width, boundary_weight, instance_sep_weight)
        self.use_focal = bool(use_focal)
        self.focal_gamma = focal_gamma
        self._cw_dev: Optional[torch.Tensor] = None
        self._cw_src: Optional[torch.Tensor] = None
        self._dev_weights: Optional[torch.Tensor] = None   # set by AdaptiveBoundaryLoss
        self._force_tiled = False
        self.last: Optional[dict] = None   # the last call's weight map and d2 (device tensors)

    def _class_weights_on(self, dev) -> Optional[torch.Tensor]:
        cw = self.class_weights
        if cw is None:
            return None
        if tuple(cw.shape) != (3,):
            raise ValueError(f"class_weights: expected 3 class weights, got shape {tuple(cw.shape)}")
        if self._cw_dev is None or self._cw_dev.device != dev or self._cw_src is not cw:
            self._cw_dev, self._cw_src = cw.detach().to(device=dev, dtype=torch.float32).contiguous(), cw
        return self._cw_dev

    def forward(self, predictions: torch.Tensor, targets: torch.Tensor, instance_info: InstanceInfo = None):
        if predictions.dim() != 4:
            raise ValueError(f"Expected 4D predictions, got shape {tuple(predictions.shape)}")
        if not predictions.is_cuda:
            raise RuntimeError("hiseg DistanceAwareSegmentationLoss runs on the GPU only (got a CPU tensor)")
        N, C, H, W = predictions.shape
        if C != 3:
            raise ValueError(f"DistanceAwareSegmentationLoss: expected 3 classes, got {C}")
        if tuple(targets.shape) != (N, H, W):
            raise ValueError(f"targets: expected [{N},{H},{W}], got {tuple(targets.shape)}")
        dev = predictions.device
        inst, present = _instance_maps(instance_info, N, H, W, dev)
        g = self.weight_generator
        handle = {"width": int(g.boundary_width), "boundary_weight": float(g.boundary_weight),
                  "instance_sep_weight": float(g.instance_sep_weight), "dev_weights": self._dev_weights,
                  "inst": inst, "present": present, "class_weights": self._class_weights_on(dev),
                  "use_focal": self.use_focal, "focal_gamma": self.focal_gamma, "ce_weight": self.ce_weight,
                  "dice_weight": self.dice_weight, "force_tiled": self._force_tiled}
        total, out = _DistanceLossFunction.apply(handle, predictions.float().contiguous(),
                                                 targets.to(device=dev, dtype=torch.int64).contiguous())
        self.last = {"weights": handle["weights"], "d2": handle["d2"]}
        return total, LazyDistanceLossDict(out)


class AdaptiveBoundaryLoss(nn.Module):
    """distance_aware_loss.py:313-373: the boundary and instance weights are nn.Parameters clamped to
    [min_weight, max_weight] before every call.  The clamp runs on the device into the two-float buffer the weight
    kernel reads (the reference calls .item() four times per step); the loss dict reports the unclamped values."""

    def __init__(self, base_loss: DistanceAwareSegmentationLoss, adaptation_rate: float = 0.01,
                 min_weight: float = 1.0, max_weight: float = 5.0):
        super().__init__()
        self.base_loss = base_loss
        self.adaptation_rate = adaptation_rate
        self.min_weight = min_weight
        self.max_weight = max_weight
        self.boundary_weight = nn.Parameter(torch.tensor(base_loss.weight_generator.boundary_weight))
        self.instance_weight = nn.Parameter(torch.tensor(base_loss.weight_generator.instance_sep_weight))
        self._buf: Optional[torch.Tensor] = None

    def forward(self, predictions: torch.Tensor, targets: torch.Tensor, instance_info: InstanceInfo = None):
        if not predictions.is_cuda:
            raise RuntimeError("hiseg AdaptiveBoundaryLoss runs on the GPU only (got a CPU tensor)")
        dev = predictions.device
        if self._buf is None or self._buf.device != dev:
            self._buf = torch.empty(2, dtype=torch.float32, device=dev)
        raw = torch.stack([self.boundary_weight.detach(), self.instance_weight.detach()]).to(
            device=dev, dtype=torch.float32)
        torch.clamp(raw, self.min_weight, self.max_weight, out=self._buf)
        self.base_loss._dev_weights = self._buf
        try:
            total, d = self.base_loss(predictions, targets, instance_info)
        finally:
            self.base_loss._dev_weights = None
        return total, LazyDistanceLossDict(torch.cat([d._out, raw]), ("boundary_weight", "instance_weight"))


def create_distance_aware_loss(pixel_ratios: dict, boundary_width: int = 5, boundary_weight: float = 2.0,
                               instance_sep_weight: float = 3.0, ce_weight: float = 1.0, dice_weight: float = 1.0,
                               adaptive: bool = False, device: str = "cpu",
                               separation_aware_weights: Optional[dict] = None, use_focal: bool = False,
                               focal_gamma: float = 2.0) -> nn.Module:
    """distance_aware_loss.py:376-437 with the class weights of losses.py:231-263 (log-scaled inverse pixel ratios,
    normalised to sum 3; ``separation_aware_weights`` replaces them as given)."""
    if separation_aware_weights is not None:
        weights = separation_aware_weights
    else:
        eps = 1e-3
        weights = {k: torch.log(torch.tensor(1.0 / (pixel_ratios[k] + eps)))
                   for k in ("background", "target", "non_target")}
        weight_sum = sum(weights.values())
        weights = {k: v / weight_sum * 3.0 for k, v in weights.items()}
    class_weights = torch.tensor([weights["background"], weights["target"], weights["non_target"]],
                                 dtype=torch.float32).to(device)
    loss = DistanceAwareSegmentationLoss(class_weights=class_weights, ce_weight=ce_weight, dice_weight=dice_weight,
                                         boundary_width=boundary_width, boundary_weight=boundary_weight,
                                         instance_sep_weight=instance_sep_weight, use_focal=use_focal,
                                         focal_gamma=focal_gamma)
    return AdaptiveBoundaryLoss(loss) if adaptive else loss
