"""Training checkpoints in the reference's format (train_advanced.py:1592-1599 save, :1204-1246 resume).

A checkpoint is ``{'epoch', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'best_miou',
'config'}``: the model keys are the reference's (hiseg keeps its module tree), the optimizer state is
torch.optim.AdamW's layout (hiseg.FusedAdamW reads and writes it), the scheduler state is the torch
scheduler's own.  So a run can resume from a reference checkpoint, and the reference can resume from a
hiseg one.  Files are read with the non-executing loader (``weights_only=True``), unlike the reference.

``load_teacher_checkpoint`` restates the distillation teacher's loading (train_advanced.py:428-508), and
``save_checkpoint`` of a ``DistillationModelWrapper`` stores the student alone (:1281-1290).

``save_distillation_checkpoint`` / ``resume_distillation_checkpoint`` are the UNet (B7 -> B0) distillation run's
layout (train_distillation_staged.py:1693-1719 save, :1351-1467 resume), which adds the adaptive-distillation
state of the loss, the cached teacher mIoU and the progressive-unfreeze state.
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn


def save_checkpoint(path: str, model: nn.Module, optimizer, epoch: int, best_miou: float = 0.0,
                    scheduler=None, config: Optional[dict] = None) -> dict:
    """train_advanced.py:1592-1599 (the dict it saves each epoch)."""
    from .kd import DistillationModelWrapper
    if isinstance(model, DistillationModelWrapper):   # train_advanced.py:1281-1290: the student only
        model = model.get_student()
    # cloned: hiseg parameters are views into one flat training buffer
    ck = {"epoch": int(epoch), "model_state_dict": {k: v.detach().clone() for k, v in model.state_dict().items()},
          "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else None,
          "scheduler_state_dict": scheduler.state_dict() if scheduler is not None else None,
          "best_miou": float(best_miou), "config": config if config is not None else {}}
    torch.save(ck, path)
    return ck


def _reseed_output_conv(model: nn.Module) -> None:
    # train_advanced.py:1230-1241: channel 0 = +u (background), channel 1 = -u, zero bias
    pu = getattr(model, "pretrained_unet", None)
    oc = getattr(pu, "output_conv", None)
    if oc is None:
        return
    with torch.no_grad():
        oc.weight.data[0, 0, 0, 0] = 1.0
        oc.weight.data[1, 0, 0, 0] = -1.0
        oc.bias.data.zero_()


def resume_from_checkpoint(path: str, model: nn.Module, optimizer=None, scheduler=None,
                           map_location="cpu") -> Tuple[int, float]:
    """train_advanced.py:1204-1246: strict load with a non-strict fallback, optimizer state, epoch + 1,
    best_miou, output_conv re-seed, scheduler state.  Returns (start_epoch, best_miou)."""
    ck = torch.load(path, map_location=map_location, weights_only=True)
    sd = ck["model_state_dict"]
    try:
        model.load_state_dict(sd)
    except RuntimeError as e:
        inc = model.load_state_dict(sd, strict=False)
        warnings.warn(f"strict load failed ({str(e).splitlines()[0]}); loaded with strict=False: "
                      f"{len(inc.missing_keys)} missing, {len(inc.unexpected_keys)} unexpected keys")
    if optimizer is not None and ck.get("optimizer_state_dict") is not None:
        optimizer.load_state_dict(ck["optimizer_state_dict"])
    start_epoch = int(ck["epoch"]) + 1
    best_miou = ck.get("best_miou", 0)
    _reseed_output_conv(model)
    if scheduler is not None and ck.get("scheduler_state_dict") is not None:
        scheduler.load_state_dict(ck["scheduler_state_dict"])
    return start_epoch, best_miou


_LOSS_FN_FIELDS = ("performance_ratio", "alpha", "task_weight", "temperature", "distillation_eliminated")


def _plain(v):
    """Checkpoint metadata as plain Python values (numpy / tensor scalars become floats), so that the file loads
    with weights_only=True."""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, torch.Tensor):
        return v.item() if v.numel() == 1 else v
    if getattr(v, "shape", None) == () and hasattr(v, "item"):   # numpy scalar
        return v.item()
    return v


def save_distillation_checkpoint(path: str, model: nn.Module, optimizer, epoch: int, loss_fn,
                                 teacher_miou_cache: Optional[float], best_iou: float = 0.0, scheduler=None,
                                 train_metrics: Optional[dict] = None, val_metrics: Optional[dict] = None,
                                 config: Optional[dict] = None,
                                 progressive_unfreeze_state: Optional[dict] = None) -> dict:
    """train_distillation_staged.py:1693-1719: the per-epoch checkpoint of a UNet distillation run, with the
    reference's keys.  ``model`` is the student / teacher wrapper: ``model_state_dict`` holds ``model.student``
    alone.  ``loss_fn_state`` holds the adaptive-distillation state (performance_ratio, alpha, task_weight,
    temperature, distillation_eliminated; the reference's defaults where ``loss_fn`` lacks a field).  ``config``
    is a plain dict (the reference stores ``config.__dict__``, which only its executing loader can read)."""
    # :1711-1717; the reference's default for a missing alpha is the configured distillation weight (0.05 in
    # create_unet_distillation_model)
    defaults = {"performance_ratio": 1.0, "alpha": 0.05, "task_weight": 0.7, "temperature": 1.0,
                "distillation_eliminated": False}
    state = {k: getattr(loss_fn, k, defaults[k]) for k in _LOSS_FN_FIELDS}
    state = {k: bool(v) if k == "distillation_eliminated" else float(v) for k, v in state.items()}
    # cloned: hiseg parameters are views into one flat training buffer
    ck = {"epoch": int(epoch),
          "model_state_dict": {k: v.detach().clone() for k, v in model.student.state_dict().items()},
          "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else None,
          "scheduler_state_dict": scheduler.state_dict() if scheduler is not None else None,
          "train_metrics": _plain(train_metrics if train_metrics is not None else {}),
          "val_metrics": _plain(val_metrics if val_metrics is not None else {}),
          "best_iou": float(best_iou),
          "config": _plain(config if config is not None else {}),
          "progressive_unfreeze_state": _plain(progressive_unfreeze_state),
          "loss_fn_state": state,
          "teacher_miou_cache": None if teacher_miou_cache is None else float(teacher_miou_cache)}
    torch.save(ck, path)
    return ck


def resume_distillation_checkpoint(path: str, model: nn.Module, loss_fn, optimizer=None, scheduler=None,
                                   encoder_lr_scale: float = 0.1, map_location="cpu") -> Dict[str, object]:
    """train_distillation_staged.py:1351-1467, in its order: student weights, ``start_epoch = epoch + 1``,
    ``best_iou``, the loss function's adaptive state (a missing field takes the reference's default; its default
    for ``alpha``, the configured distillation weight, is ``loss_fn.initial_alpha`` here; a checkpoint without
    ``loss_fn_state`` leaves the loss as it is), ``teacher_miou_cache`` (None when absent), then
    ``model.unfreeze_encoder_blocks(blocks_unfrozen, encoder_lr_scale)`` when the checkpoint had encoder blocks
    unfrozen, and only then the optimizer and scheduler states.

    The optimizer a checkpoint with unfrozen blocks was saved from has a second parameter group for them; building
    that optimizer (decoder group at the base rate, unfrozen group at ``encoder_lr_scale`` times it, :1406-1426) is
    the caller's part: pass ``optimizer=None``, rebuild it from the returned ``blocks_unfrozen`` and load
    ``torch.load(path, weights_only=True)['optimizer_state_dict']`` into it.  An optimizer or scheduler state that
    does not fit is reported with a warning and skipped, as the reference does.

    Returns ``{'start_epoch', 'best_iou', 'teacher_miou_cache', 'blocks_unfrozen'}``."""
    ck = torch.load(path, map_location=map_location, weights_only=True)
    model.student.load_state_dict(ck["model_state_dict"])
    start_epoch = int(ck["epoch"]) + 1
    best_iou = ck.get("best_iou", 0)
    if "loss_fn_state" in ck:
        st = ck["loss_fn_state"]
        defaults = {"performance_ratio": 1.0, "alpha": getattr(loss_fn, "initial_alpha", None), "task_weight": 0.7,
                    "temperature": 1.0, "distillation_eliminated": False}
        for k in _LOSS_FN_FIELDS:
            if hasattr(loss_fn, k):
                setattr(loss_fn, k, st.get(k, defaults[k]))
    teacher_miou_cache = ck.get("teacher_miou_cache")
    pu = ck.get("progressive_unfreeze_state")
    blocks_unfrozen = int(pu.get("blocks_unfrozen", 0)) if pu else 0
    if blocks_unfrozen > 0:
        model.unfreeze_encoder_blocks(blocks_unfrozen, encoder_lr_scale)
    if optimizer is not None and ck.get("optimizer_state_dict") is not None:
        try:
            optimizer.load_state_dict(ck["optimizer_state_dict"])
        except Exception as e:   # :1429-1434, :1448-1459
            warnings.warn(f"could not restore the optimizer state: {e}")
    if scheduler is not None and ck.get("scheduler_state_dict") is not None:
        try:
            scheduler.load_state_dict(ck["scheduler_state_dict"])
        except Exception as e:   # :1461-1465
            warnings.warn(f"could not restore the scheduler state: {e}")
    return {"start_epoch": start_epoch, "best_iou": best_iou, "teacher_miou_cache": teacher_miou_cache,
            "blocks_unfrozen": blocks_unfrozen}


def load_teacher_checkpoint(path: str, teacher_model: nn.Module, map_location="cpu") -> Dict[str, List[str]]:
    """train_advanced.py:428-508: the distillation teacher's weights from a training checkpoint.

    An old-format checkpoint (it has ``pretrained_unet.norm_mean``) gets its ``pretrained_unet.`` keys remapped to
    ``pretrained_unet.model.``; keys the model does not have, or has with another shape, are dropped and the rest
    is loaded with ``strict=False``; when ``pretrained_unet.output_conv.weight`` was in neither the checkpoint nor
    the loaded keys, output_conv becomes (-u, +u) with a zero bias (:495-508).  Returns the loaded, skipped
    (shape mismatch), missing and unexpected key lists."""
    ck = torch.load(path, map_location=map_location, weights_only=True)
    state_dict = ck["model_state_dict"]
    if "pretrained_unet.norm_mean" in state_dict:
        remapped = {}
        for key, value in state_dict.items():
            if key.startswith("pretrained_unet."):
                remapped["pretrained_unet.model." + key.split(".", 1)[1]] = value
            else:
                remapped[key] = value
    else:
        remapped = state_dict
    model_state = teacher_model.state_dict()
    filtered, skipped = {}, []
    for key, value in remapped.items():
        if key in model_state:
            if model_state[key].shape == value.shape:
                filtered[key] = value
            else:
                skipped.append(key)
    inc = teacher_model.load_state_dict(filtered, strict=False)
    if skipped or inc.missing_keys:
        warnings.warn(f"teacher checkpoint: {len(skipped)} keys skipped for their shape, "
                      f"{len(inc.missing_keys)} missing")
    oc = getattr(getattr(teacher_model, "pretrained_unet", None), "output_conv", None)
    oc_key = "pretrained_unet.output_conv.weight"
    if oc is not None and oc_key not in filtered and oc_key not in state_dict:
        with torch.no_grad():
            oc.weight.zero_()
            oc.weight[0, 0] = -1.0
            oc.weight[1, 0] = 1.0
            oc.bias.zero_()
    return {"loaded": list(filtered), "skipped": skipped, "missing": list(inc.missing_keys),
            "unexpected": list(inc.unexpected_keys)}
