"""Validation half of the B7 -> B0 UNet distillation (train_distillation_staged.py:369-581 evaluate,
:1633-1666 adaptive-weight update).

The reference thresholds the student and teacher logits and the masks into float tensors and reduces about 40
elementwise products of them per batch, with about six ``.item()`` synchronisations.  Every number it reports is
a function of eight counts per sample -- the joint histogram of the (mask, teacher, student) bits -- so here one
HIP pass per batch (``hiseg_binary_seg_stats``, include/hiseg_metrics.h) builds that histogram on the device and
nothing synchronises inside the loop: histograms, loss totals and the lazily held loss dicts come to the host in
one copy after the last batch, where the reference's float arithmetic (torch CPU float32 ops in its order, Python
float sums over the batches) is reproduced exactly.

Foreground predicate (stated in include/hiseg_metrics.h): a logit x is foreground iff ``x > 1.5 * 2**-24`` in
float32, which is ``sigmoid(x) > 0.5`` under correctly rounded float32 arithmetic -- 0.0, -0.0, NaN and negative
values are background, +inf and every x >= 1e-6 foreground; inside the open band (0, 1e-6) torch's own answer
depends on its sigmoid implementation and no parity is claimed.  bfloat16 logits are widened to float32 first
(torch's bfloat16 sigmoid rounds to bfloat16 instead).  A mask pixel is foreground iff ``mask > 0.5``.
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from . import _lib as L

_HISEG_U8 = 2   # include/hiseg_metrics.h
_LOSS_KEYS = ("kl_loss", "mse_loss", "bce_loss", "dice_loss")


def binary_seg_stats(student: torch.Tensor, teacher: Optional[torch.Tensor], masks: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-sample joint histogram int64 [B, 8]: ``out[b, 4*m + 2*t + s]`` counts the pixels of sample b with mask
    bit m, teacher bit t and student bit s (``teacher=None``: t = s).  Logits [B, ...] float32 / bfloat16 (other
    dtypes are widened to float32), masks float32 or uint8 / bool (other dtypes are converted to float32), all of
    one shape up to singleton axes.  Accumulates into ``out`` when given.  Runs on the device, never
    synchronises."""
    tensors = (student, masks) if teacher is None else (student, teacher, masks)
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("hiseg distillation metrics run on the GPU only (got a CPU tensor)")
    B = student.shape[0] if student.dim() else 0
    HW = student.numel() // B if B else 0
    for name, t in (("teacher", teacher), ("masks", masks)):
        if t is not None and (t.dim() == 0 or t.shape[0] != B or t.numel() != B * HW):
            raise ValueError(f"binary_seg_stats: student {tuple(student.shape)} vs {name} {tuple(t.shape)}")
    if out is None:
        out = torch.zeros(B, 8, dtype=torch.int64, device=student.device)
    elif tuple(out.shape) != (B, 8) or out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"binary_seg_stats: out must be a contiguous int64 [{B}, 8] device tensor")
    if B == 0 or HW == 0:
        return out

    def logits(x):
        x = x.detach()
        return (x if x.dtype in (torch.float32, torch.bfloat16) else x.float()).contiguous()

    s = logits(student)
    t = logits(teacher) if teacher is not None else None
    m = masks.detach()
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    elif m.dtype not in (torch.float32, torch.uint8):
        m = m.float()
    m = m.contiguous()
    from .ops import hdtype
    L.check(L.lib().hiseg_binary_seg_stats(
        s.data_ptr(), hdtype(s.dtype), t.data_ptr() if t is not None else None,
        hdtype(t.dtype) if t is not None else 0, m.data_ptr(), _HISEG_U8 if m.dtype == torch.uint8 else 0,
        B, HW, out.data_ptr(), L.stream_ptr(student.device)), "binary_seg_stats")
    return out


def _miou(c: torch.Tensor, bit: int) -> torch.Tensor:
    """:453-465 / :472-484 for the predictions held in bit ``bit`` (0: student, 1: teacher) of the histogram
    index: per-sample (background IoU + foreground IoU) / 2 in float32.  The reference's sums of 0/1 floats are
    exact integers in float32 (below 2**24 pixels per sample), so they are the counts."""
    def n(pred: int, mask: int) -> torch.Tensor:
        ks = [k for k in range(8) if (k >> bit) & 1 == pred and (k >> 2) & 1 == mask]
        return c[:, ks].sum(1).to(torch.float32)

    bg_tp, bg_fp, bg_fn = n(0, 0), n(0, 1), n(1, 0)
    bg_iou = bg_tp / (bg_tp + bg_fp + bg_fn + 1e-6)
    fg_tp, fg_fp, fg_fn = n(1, 1), n(1, 0), n(0, 1)
    fg_iou = fg_tp / (fg_tp + fg_fp + fg_fn + 1e-6)
    return (bg_iou + fg_iou) / 2.0


def _value(v) -> float:
    return v.item() if isinstance(v, torch.Tensor) else v


def distill_metrics_from_counts(counts_per_batch: Sequence, loss_totals: Sequence[float],
                                loss_dicts: Sequence[Mapping], teacher_miou_cache: Optional[float] = None,
                                has_teacher: bool = True) -> Dict[str, float]:
    """The reference's metric arithmetic (:437-441, :451-525) from one [B, 8] histogram per batch (in evaluation
    order; tensors, arrays or nested lists), the per-batch ``loss.item()`` values and loss dicts.  Pure host
    arithmetic.  ``teacher_miou_cache`` given: the teacher's mIoU is not computed and the cached value is
    reported (:505-506).  ``has_teacher=False`` (``model.teacher is None``): the teacher's predictions are the
    student's (:447-448), so teacher_miou is student_miou and the agreement is 1."""
    num_batches = len(counts_per_batch)
    if num_batches == 0:
        raise ZeroDivisionError("distillation evaluation: no batches (the reference divides by num_batches = 0)")
    if not (len(loss_totals) == len(loss_dicts) == num_batches):
        raise ValueError("distill_metrics_from_counts: one loss total and one loss dict per batch")
    use_cached = teacher_miou_cache is not None
    total_loss = 0
    sums = {k: 0 for k in _LOSS_KEYS}
    total_student_iou = total_teacher_iou = total_agreement = 0
    for counts, total, d in zip(counts_per_batch, loss_totals, loss_dicts):
        c = torch.as_tensor(counts).to("cpu", torch.int64).reshape(-1, 8)
        total_loss += _value(total)
        for k in _LOSS_KEYS:
            sums[k] += _value(d.get(k, 0))
        student_miou = _miou(c, 0)
        total_student_iou += student_miou.mean().item()
        if not use_cached:
            total_teacher_iou += (_miou(c, 1) if has_teacher else student_miou).mean().item()
        pixels = c.sum(1)
        agree = c[:, [0, 3, 4, 7]].sum(1) if has_teacher else pixels          # student bit == teacher bit
        agreement = agree.to(torch.float32) / pixels.to(torch.float32)         # .float().mean(dim=(1, 2, 3))
        total_agreement += agreement.mean().item()
    if use_cached:
        final_teacher_miou = teacher_miou_cache
    elif not has_teacher:
        final_teacher_miou = total_student_iou / num_batches
    else:
        final_teacher_miou = total_teacher_iou / num_batches
    return {
        "total_loss": total_loss / num_batches,
        "kl_loss": sums["kl_loss"] / num_batches,
        "mse_loss": sums["mse_loss"] / num_batches,
        "bce_loss": sums["bce_loss"] / num_batches,
        "dice_loss": sums["dice_loss"] / num_batches,
        "student_miou": total_student_iou / num_batches,
        "teacher_miou": final_teacher_miou,
        "agreement": total_agreement / num_batches,
        "miou_diff": (total_student_iou / num_batches) - final_teacher_miou,
        "iou": total_student_iou / num_batches,
    }


def evaluate_distillation(model, dataloader, loss_fn, device, epoch: int = 0, writer=None, visualize_dir=None,
                          teacher_miou_cache: Optional[float] = None, student_name: str = "Student",
                          teacher_name: str = "Teacher") -> Dict[str, float]:
    """train_distillation_staged.py:369-581 (the reference's ``evaluate``, its argument order and returned keys):
    ``model(images) -> (student, teacher)`` with a ``.teacher`` attribute (None: fine-tuning mode),
    ``loss_fn(student, teacher, masks) -> (loss, loss_dict)``, batches are ``(images, masks)``.  One histogram
    launch per batch and no host synchronisation inside the loop; ``writer`` (anything with ``add_scalar``)
    receives the nine Val/* scalars.  The reference's console summary and matplotlib panels are not produced."""
    if visualize_dir is not None:
        warnings.warn("hiseg.evaluate_distillation does not draw the student / teacher visualisation panels "
                      "(matplotlib figures); the metrics are returned")
    model.eval()
    has_teacher = getattr(model, "teacher", None) is not None
    counts: List[torch.Tensor] = []
    losses: List[torch.Tensor] = []
    dicts: List[Mapping] = []
    with torch.no_grad():
        for images, masks in dataloader:
            images = images.to(device)
            masks = masks.to(device)
            student_output, teacher_output = model(images)
            loss, loss_dict = loss_fn(student_output, teacher_output, masks)
            counts.append(binary_seg_stats(student_output, teacher_output if has_teacher else None, masks))
            losses.append(loss.detach().reshape(()))
            dicts.append(loss_dict)
    if not counts:
        raise ZeroDivisionError("evaluate_distillation: empty dataloader (the reference divides by num_batches = 0)")
    # one transfer: histograms (exact in float64 below 2**53), loss totals and every lazily held loss dict
    from .distill import _LazyDict
    dev = counts[0].device
    lazy = [d for d in dicts if isinstance(d, _LazyDict) and d._vals is None]
    parts = [c.reshape(-1).to(torch.float64) for c in counts]
    parts.append(torch.stack([t.to(dev).float() for t in losses]).to(torch.float64))
    parts += [d._out.detach().to(dev).reshape(-1).to(torch.float64) for d in lazy]
    host = torch.cat(parts).cpu()
    pos = 0
    host_counts = []
    for c in counts:
        host_counts.append(host[pos:pos + c.numel()].to(torch.int64).reshape(-1, 8))
        pos += c.numel()
    totals = host[pos:pos + len(losses)].tolist()
    pos += len(losses)
    for d in lazy:
        n = d._out.numel()
        d._materialise(host[pos:pos + n].tolist())
        pos += n
    metrics = distill_metrics_from_counts(host_counts, totals, dicts, teacher_miou_cache, has_teacher)
    if writer:
        for tag, key in (("Val/Loss", "total_loss"), ("Val/KL_Loss", "kl_loss"), ("Val/MSE_Loss", "mse_loss"),
                         ("Val/BCE_Loss", "bce_loss"), ("Val/Dice_Loss", "dice_loss"),
                         ("Val/Student_mIoU", "student_miou"), ("Val/Teacher_mIoU", "teacher_miou"),
                         ("Val/Agreement", "agreement"), ("Val/mIoU_Diff", "miou_diff")):
            writer.add_scalar(tag, metrics[key], epoch)
    return metrics


def update_adaptive_distillation(loss_fn, val_metrics: Mapping, teacher_miou_cache: Optional[float],
                                 min_alpha: float = 0.0, amplification_factor: float = 20.0,
                                 zero_distillation_threshold: float = 0.03) -> Tuple[float, Optional[str]]:
    """train_distillation_staged.py:1633-1666 for a run with distillation enabled: fills the teacher-mIoU cache
    from the first evaluation, feeds ``val_metrics['student_miou']`` and the cached teacher value to
    ``loss_fn.update_distillation_weight`` and returns ``(teacher_miou_cache, message)`` with the reference's log
    text -- weights changed, distillation just eliminated, or distillation remains eliminated -- or None.  The
    reference reaches its "remains ELIMINATED" text only when a weight changed while already eliminated, which
    its own update never does; here every call after the elimination returns it."""
    if teacher_miou_cache is None:
        teacher_miou_cache = val_metrics["teacher_miou"]
    if not hasattr(loss_fn, "update_distillation_weight"):
        return teacher_miou_cache, None
    old_alpha = loss_fn.alpha
    old_task_weight = loss_fn.task_weight
    new_alpha = loss_fn.update_distillation_weight(
        student_iou=val_metrics["student_miou"], teacher_iou=teacher_miou_cache, min_alpha=min_alpha,
        amplification_factor=amplification_factor, zero_distillation_threshold=zero_distillation_threshold)
    changed = old_alpha != new_alpha or old_task_weight != loss_fn.task_weight
    eliminated = bool(getattr(loss_fn, "distillation_eliminated", False)) and \
        bool(getattr(loss_fn, "adaptive_distillation", True))
    ratio = getattr(loss_fn, "performance_ratio", 1.0)
    if eliminated and changed and old_alpha != 0.0:
        msg = (f"  🎯 Distillation PERMANENTLY ELIMINATED: Student/Teacher ratio = {ratio:.4f}, "
               f"Student surpassed teacher by {(ratio - 1.0) * 100:.1f}%, "
               f"Now using 100% ground truth labels FOREVER!")
    elif eliminated:
        msg = (f"  🎯 Distillation remains ELIMINATED: Student/Teacher ratio = {ratio:.4f}, "
               f"Continuing with 100% ground truth labels")
    elif changed:
        amplified_diff = (ratio - 1.0) * amplification_factor
        msg = (f"  Adaptive distillation: Student/Teacher ratio = {ratio:.4f}, "
               f"amplified_diff = {amplified_diff:.3f}, "
               f"α: {old_alpha:.3f} → {new_alpha:.3f}, "
               f"task_weight: {old_task_weight:.3f} → {loss_fn.task_weight:.3f}")
    else:
        msg = None
    return teacher_miou_cache, msg
