"""Teacher -> student knowledge distillation of the ROI model on libhiseg (advanced/knowledge_distillation.py,
train_advanced.py:369-522, :634-643).

Same surface as the reference module: ``DistillationLoss(base_loss_fn, temperature, alpha, ...)`` with
``forward(student_outputs, teacher_outputs, targets, aux_outputs=None) -> (total, loss_dict)`` and
``DistillationModelWrapper(teacher_model, student_model, freeze_teacher=True)``.  The three KL terms (logits,
bg/fg, target/non-target) run as one fused HIP forward and one fused HIP backward (include/hiseg_kd.h); the
temperature and alpha live in device scalars that the kernels and the alpha mix read, so a captured step follows a
temperature / alpha schedule without a re-capture, and nothing in a step synchronises with the host (the reference
calls ``.item()`` per term).  ``loss_dict`` is lazy: one device->host copy on first access, shared with the base
loss's own lazy dict.
"""
from __future__ import annotations

from collections.abc import Mapping
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from .losses import LazyLossDict

NOUT = 4   # include/hiseg_kd.h HISEG_KD_NOUT
_TERM_KEYS = ("distill_logits", "distill_bg_fg", "distill_target")
_AUX_KEYS = ("bg_fg_logits", "target_nontarget_logits")


class LazyDistillationLossDict(Mapping):
    """dict[str, float] of DistillationLoss in the reference's key order: ``base_<k>`` for the base dict, the
    terms that ran, ``distill_total``, ``base_total``, ``total``.  ``vec`` (device f32) holds the four kernel
    outputs, base_total, total and, after them, the device outputs of a lazy base dict; the first access copies it
    to the host once."""

    def __init__(self, vec: torch.Tensor, terms, base_dict):
        self._vec, self._terms, self._base, self._vals = vec, tuple(terms), base_dict, None

    def _materialise(self) -> Dict[str, float]:
        if self._vals is None:
            host = self._vec.detach().cpu().tolist()
            base = self._base
            if isinstance(base, LazyLossDict):
                base = base._materialise(host[NOUT + 2:])
            v = {f"base_{k}": val for k, val in base.items()}
            for i, k in enumerate(_TERM_KEYS):
                if self._terms[i]:
                    v[k] = host[1 + i]
            v["distill_total"] = host[0] if any(self._terms) else 0
            v["base_total"] = host[NOUT]
            v["total"] = host[NOUT + 1]
            self._vals = v
        return self._vals

    def __getitem__(self, k):
        return self._materialise()[k]

    def __iter__(self):
        return iter(self._materialise())

    def __len__(self):
        return len(self._materialise())

    def copy(self):
        return dict(self._materialise())


class _KdFunction(torch.autograd.Function):
    """out[0] (the sum of the enabled terms) as a differentiable scalar, and the four outputs."""

    @staticmethod
    def forward(ctx, dev_T, s0, t0, s1, t1, s2, t2):
        lib = L.lib()
        first = next(t for t in (s0, s1, s2) if t is not None)
        N, _, H, W = first.shape
        dev = first.device
        ws = torch.empty(int(lib.hiseg_kd_ws(N, H, W)), dtype=torch.float32, device=dev)
        out = torch.empty(NOUT, dtype=torch.float32, device=dev)

        def p(t):
            return t.data_ptr() if t is not None else None
        L.check(lib.hiseg_kd_loss_fwd(p(s0), p(t0), p(s1), p(t1), p(s2), p(t2), N, H, W, 0.0, dev_T.data_ptr(),
                                      ws.data_ptr(), out.data_ptr(), L.stream_ptr()), "kd_loss_fwd")
        ctx.save_for_backward(dev_T, s0, t0, s1, t1, s2, t2)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g_total, _g_out):
        dev_T, s0, t0, s1, t1, s2, t2 = ctx.saved_tensors
        first = next(t for t in (s0, s1, s2) if t is not None)
        N, _, H, W = first.shape
        g = g_total.contiguous().float()
        d0, d1, d2 = (torch.empty_like(t) if t is not None else None for t in (s0, s1, s2))

        def p(t):
            return t.data_ptr() if t is not None else None
        L.check(L.lib().hiseg_kd_loss_bwd(p(s0), p(t0), p(s1), p(t1), p(s2), p(t2), N, H, W, 0.0, dev_T.data_ptr(),
                                          g.data_ptr(), p(d0), p(d1), p(d2), L.stream_ptr()), "kd_loss_bwd")
        return None, d0, None, d1, None, d2, None


def _pair(name: str, s: torch.Tensor, t: torch.Tensor, channels: int):
    if s.dim() != 4 or s.shape[1] != channels or tuple(t.shape) != tuple(s.shape):
        raise ValueError(f"DistillationLoss: {name}: student {tuple(s.shape)} teacher {tuple(t.shape)} "
                         f"(expect the same [N,{channels},H,W])")
    if not s.is_cuda or not t.is_cuda:
        raise RuntimeError("hiseg DistillationLoss runs on the GPU only (got a CPU tensor)")
    return s.float().contiguous(), t.detach().to(s.device).float().contiguous()


class DistillationLoss(nn.Module):
    """knowledge_distillation.py:10-134; arguments as the reference.  ``distill_features`` and
    ``feature_match_layers`` are stored and unused, as there (its forward never reads them)."""

    def __init__(self, base_loss_fn: nn.Module, temperature: float = 4.0, alpha: float = 0.7,
                 distill_logits: bool = True, distill_features: bool = False,
                 feature_match_layers: Optional[list] = None):
        super().__init__()
        self.base_loss_fn = base_loss_fn
        self._temperature = float(temperature)
        self._alpha = float(alpha)
        self.distill_logits = distill_logits
        self.distill_features = distill_features
        self.feature_match_layers = feature_match_layers or []
        self._dev: Optional[torch.Tensor] = None   # device f32 [temperature, alpha], updated in place

    # -- schedule values: host attributes backed by the device scalars the kernels and the alpha mix read
    def _set(self, index: int, value: float):
        if self._dev is not None:
            self._dev[index].fill_(value)

    @property
    def temperature(self) -> float:
        return self._temperature

    @temperature.setter
    def temperature(self, value: float):
        if not float(value) > 0.0:
            raise ValueError(f"DistillationLoss: temperature must be > 0, got {value}")
        self._temperature = float(value)
        self._set(0, self._temperature)

    @property
    def alpha(self) -> float:
        return self._alpha

    @alpha.setter
    def alpha(self, value: float):
        self._alpha = float(value)
        self._set(1, self._alpha)

    def device_scalars(self, device) -> torch.Tensor:
        """The device f32 [temperature, alpha] on ``device`` (created on the first call; not while capturing)."""
        device = torch.device(device)
        if self._dev is None or self._dev.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DistillationLoss: the first call cannot be captured (run it eagerly first)")
            self._dev = torch.tensor([self._temperature, self._alpha], dtype=torch.float32, device=device)
        return self._dev

    def forward(self, student_outputs: Any, teacher_outputs: Any, targets: torch.Tensor,
                aux_outputs: Optional[Dict] = None) -> Tuple[torch.Tensor, Mapping]:
        if isinstance(student_outputs, tuple):
            student_logits, student_aux = student_outputs
        else:
            student_logits, student_aux = student_outputs, aux_outputs
        if isinstance(teacher_outputs, tuple):
            teacher_logits, teacher_aux = teacher_outputs
        else:
            teacher_logits, teacher_aux = teacher_outputs, None
        if not student_logits.is_cuda:
            raise RuntimeError("hiseg DistillationLoss runs on the GPU only (got a CPU tensor)")
        pairs = [None, None, None]
        if self.distill_logits:
            pairs[0] = _pair("logits", student_logits, teacher_logits, 3)
        if student_aux is not None and teacher_aux is not None:
            for i, k in enumerate(_AUX_KEYS):
                if k in student_aux and k in teacher_aux:
                    pairs[1 + i] = _pair(k, student_aux[k], teacher_aux[k], 2)
        shapes = {(p[0].shape[0],) + tuple(p[0].shape[2:]) for p in pairs if p is not None}
        if len(shapes) > 1:
            raise ValueError(f"DistillationLoss: the heads disagree on [N,H,W]: {sorted(shapes)}")

        if student_aux is not None:
            base_loss, base_dict = self.base_loss_fn(student_logits, targets, student_aux)
        else:
            base_loss, base_dict = self.base_loss_fn(student_logits, targets)

        dev = student_logits.device
        scal = self.device_scalars(dev)
        alpha = scal[1]
        terms = tuple(p is not None for p in pairs)
        base_loss = base_loss.to(device=dev, dtype=torch.float32)
        if any(terms):
            flat = [t for p in pairs for t in (p if p is not None else (None, None))]
            distill, out = _KdFunction.apply(scal[0:1], *flat)
            total = alpha * distill + (1 - alpha) * base_loss
        else:
            out = torch.zeros(NOUT, dtype=torch.float32, device=dev)
            total = (1 - alpha) * base_loss
        parts = [out, base_loss.detach().reshape(1), total.detach().reshape(1)]
        if isinstance(base_dict, LazyLossDict):   # its device outputs ride in the same host copy
            parts.append(base_dict._out.detach().to(torch.float32))
        return total, LazyDistillationLossDict(torch.cat(parts), terms, base_dict)


class DistillationModelWrapper(nn.Module):
    """knowledge_distillation.py:137-207: the student (train engine in train mode) beside a frozen teacher, which
    runs the eval-mode inference engine under ``no_grad``.  State-dict keys are ``teacher.*`` / ``student.*``.

    ``overlap_teacher``: True (the default) runs the teacher on the process's side stream (hiseg.streams, role
    ``teacher``), forked from and joined back into the caller's stream with events, so the student forward proceeds
    beside it; False runs it on the caller's stream after the student.  Same kernels on the same inputs either way:
    the outputs are bit-identical.  Overlapped measured 4 % faster per B0 train step on the MI355X (DESIGN.md §4
    "Knowledge distillation of the ROI model")."""

    overlap_teacher = True

    def __init__(self, teacher_model: nn.Module, student_model: nn.Module, freeze_teacher: bool = True):
        super().__init__()
        if not freeze_teacher:
            raise NotImplementedError("hiseg DistillationModelWrapper runs a frozen teacher on the inference "
                                      "engine; a trainable teacher is not supported (DESIGN.md §7)")
        self.teacher = teacher_model
        self.student = student_model
        for param in self.teacher.parameters():
            param.requires_grad = False
        self.teacher.eval()

    def _teacher_forward(self, *args, **kwargs):
        if not self.teacher.training:
            with torch.no_grad():
                return self.teacher(*args, **kwargs)
        return self.teacher(*args, **kwargs)

    def forward(self, *args, **kwargs) -> Tuple[Any, Any]:
        tensors = [a for a in list(args) + list(kwargs.values()) if isinstance(a, torch.Tensor)]
        if self.overlap_teacher and tensors and tensors[0].is_cuda:
            from .streams import role_stream
            dev = tensors[0].device
            main = torch.cuda.current_stream(dev)
            side = role_stream("teacher", dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                teacher_outputs = self._teacher_forward(*args, **kwargs)
            student_outputs = self.student(*args, **kwargs)
            main.wait_stream(side)
            for t in _tensors_of(teacher_outputs):
                t.record_stream(main)
            return student_outputs, teacher_outputs
        student_outputs = self.student(*args, **kwargs)
        teacher_outputs = self._teacher_forward(*args, **kwargs)
        return student_outputs, teacher_outputs

    def train(self, mode: bool = True):
        """Training mode for the student only; a frozen teacher stays in eval."""
        self.student.train(mode)
        if not any(p.requires_grad for p in self.teacher.parameters()):
            self.teacher.eval()
        else:
            self.teacher.train(mode)
        return self

    def eval(self):
        self.student.eval()
        self.teacher.eval()
        return self

    def get_student(self) -> nn.Module:
        return self.student

    def get_teacher(self) -> nn.Module:
        return self.teacher


def _tensors_of(outputs):
    if isinstance(outputs, torch.Tensor):
        yield outputs
    elif isinstance(outputs, Mapping):
        for v in outputs.values():
            yield from _tensors_of(v)
    elif isinstance(outputs, (tuple, list)):
        for v in outputs:
            yield from _tensors_of(v)


def create_distilled_rgb_hierarchical_model(student_kwargs: dict, teacher_checkpoint: str,
                                            teacher_encoder: str = "timm-efficientnet-b3",
                                            freeze_teacher: bool = True) -> DistillationModelWrapper:
    """train_advanced.py:369-522: the student built from ``student_kwargs``, the teacher from the same arguments
    with its own ``encoder_name`` and ``freeze_pretrained_weights=False`` (:382-407; the whole teacher is frozen by
    the wrapper), loaded from ``teacher_checkpoint`` and wrapped."""
    import os

    from .checkpoint import load_teacher_checkpoint
    from .model import create_rgb_hierarchical_model
    if not teacher_checkpoint:
        raise ValueError("Teacher checkpoint path is empty")
    if not os.path.exists(teacher_checkpoint):
        raise FileNotFoundError(f"Teacher checkpoint not found: {teacher_checkpoint}")
    student = create_rgb_hierarchical_model(**student_kwargs)
    teacher_kwargs = dict(student_kwargs)
    teacher_kwargs.update(encoder_name=teacher_encoder, freeze_pretrained_weights=False)
    teacher = create_rgb_hierarchical_model(**teacher_kwargs)
    load_teacher_checkpoint(teacher_checkpoint, teacher)
    return DistillationModelWrapper(teacher, student, freeze_teacher=freeze_teacher)
