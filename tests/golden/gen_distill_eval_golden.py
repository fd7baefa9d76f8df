"""Golden vectors of the reference's distillation validation (train_distillation_staged.py:369-581, evaluate).

Run in the build container only (the reference is at /root/reference and never leaves it):
    python tests/golden/gen_distill_eval_golden.py
Runs the reference's own evaluate on recorded batches (the method of gen_metrics_golden.py): a replay model with
a ``.teacher`` attribute returns the recorded student and teacher logits of each batch, a replay loss returns a
recorded total and loss dict, so the thresholding, IoU, agreement and averaging code of evaluate runs unchanged.
train_distillation_staged imports torch.utils.tensorboard (absent from this image; a stand-in module is installed
for the import, no writer is used) and the model modules, which import segmentation_models_pytorch
(gen_golden.py's stand-in).

Three runs over the same batches: with a teacher, with teacher_miou_cache = 0.8125, and with model.teacher = None.
Writes tests/golden/distill_eval.npz: per batch the student / teacher logits, masks, loss total and loss terms, and
per run every value evaluate returns.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402,F401  (installs the smp stand-in and the reference path)

if "torch.utils.tensorboard" not in sys.modules:
    _tb = types.ModuleType("torch.utils.tensorboard")
    _tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda s, *a, **kw: None})
    sys.modules["torch.utils.tensorboard"] = _tb
from train_distillation_staged import evaluate  # noqa: E402

LOSS_KEYS = ["kl_loss", "mse_loss", "bce_loss", "dice_loss"]
SHAPES = ((2, 16, 12), (3, 8, 8), (4, 24, 20))
CACHE = 0.8125


def make_batches(seed: int):
    """Three batches of different B and H x W.  Logits are quantised to 1/4, so exact zeros occur (background)
    and no logit lies in (0, 1e-6); the teacher follows the mask more closely than the student.  Single NaN, +inf
    and -inf logits; masks are float32 ellipses with a few pixels exactly 0.5 (background), 0.75 (foreground)
    and NaN (background).  Sample 1 of batch 1 has an all-background mask and all-background predictions."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b, h, w in SHAPES:
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
        r = torch.rand(b, 2, generator=g) * 0.4 + 0.3
        m = ((yy[None] / r[:, 0, None, None]) ** 2 + (xx[None] / r[:, 1, None, None]) ** 2 < 1).float()[:, None]
        s = torch.round((torch.randn(b, 1, h, w, generator=g) * 1.5 + (m - 0.5) * 2.0) * 4) / 4
        t = torch.round((torch.randn(b, 1, h, w, generator=g) * 1.0 + (m - 0.5) * 4.0) * 4) / 4
        out.append([s, t, m])
    s, t, m = out[0]
    s[0, 0, 1, 2] = float("nan")
    s[1, 0, 3, 4] = float("inf")
    s[1, 0, 5, 6] = float("-inf")
    t[0, 0, 2, 3] = float("nan")
    t[1, 0, 4, 5] = float("inf")
    t[0, 0, 6, 7] = float("-inf")
    m[0, 0, 8, 6] = 0.5
    m[0, 0, 8, 7] = 0.75
    m[1, 0, 8, 5] = float("nan")
    m[1, 0, 0, 0] = 0.75
    m[1, 0, 7, 6] = 0.5
    s, t, m = out[1]
    m[1] = 0.0
    s[1] = -torch.abs(s[1])
    t[1] = -torch.abs(t[1])
    for s, t, _ in out:
        for x in (s, t):
            v = x[torch.isfinite(x)]
            assert not ((v > 0) & (v < 1e-6)).any()
            assert (v == 0).any()
    return out


class _Replay(nn.Module):
    def __init__(self, batches, with_teacher=True):
        super().__init__()
        self.batches = batches
        self.teacher = nn.Identity() if with_teacher else None
        self.k = 0

    def forward(self, images):
        s, t, _ = self.batches[self.k]
        self.k += 1
        # teacher-less mode: the wrapper returns zeros for the teacher (unet_decoder_distillation.py forward)
        return s, (t if self.teacher is not None else torch.zeros_like(s))


class _ReplayLoss:
    def __init__(self, vals):
        self.vals = list(vals)
        self.k = 0

    def __call__(self, student, teacher, masks):
        total, d = self.vals[self.k]
        self.k += 1
        return torch.tensor(total), dict(d)


def main():
    batches = make_batches(11)
    rng = np.random.default_rng(5)
    loss_vals = []
    for _ in batches:
        d = {k: float(np.float32(rng.uniform(0.01, 2.0))) for k in LOSS_KEYS}
        loss_vals.append((float(np.float32(rng.uniform(0.5, 3.0))), d))
    loader = [(torch.zeros(m.shape[0], 3, 8, 8), m) for _, _, m in batches]
    runs = {
        "teacher": evaluate(_Replay(batches), loader, _ReplayLoss(loss_vals), "cpu", 0),
        "cached": evaluate(_Replay(batches), loader, _ReplayLoss(loss_vals), "cpu", 0, teacher_miou_cache=CACHE),
        "noteacher": evaluate(_Replay(batches, with_teacher=False), loader, _ReplayLoss(loss_vals), "cpu", 0),
    }
    arrays = {}
    for i, (s, t, m) in enumerate(batches):
        arrays[f"b{i}_student"] = s.numpy().astype(np.float32)
        arrays[f"b{i}_teacher"] = t.numpy().astype(np.float32)
        arrays[f"b{i}_masks"] = m.numpy().astype(np.float32)
        arrays[f"b{i}_loss_total"] = np.float64(loss_vals[i][0])
        arrays[f"b{i}_loss_terms"] = np.array([loss_vals[i][1][k] for k in LOSS_KEYS], np.float64)
    arrays["num_batches"] = np.int64(len(batches))
    arrays["loss_keys"] = np.array(LOSS_KEYS)
    arrays["teacher_miou_cache"] = np.float64(CACHE)
    keys = list(runs["teacher"])
    arrays["metric_keys"] = np.array(keys)
    for name, metrics in runs.items():
        assert list(metrics) == keys
        for k in keys:
            arrays[f"{name}_{k}"] = np.float64(metrics[k])
    np.savez_compressed(os.path.join(HERE, "distill_eval.npz"), **arrays)
    for name, metrics in runs.items():
        print(name, metrics)


if __name__ == "__main__":
    main()
