"""Distillation validation on the host: the metric arithmetic of hiseg.distill_eval against the reference's own
evaluate (tests/golden/distill_eval.npz, gen_distill_eval_golden.py), the adaptive-weight glue and the
distillation checkpoint layout (train_distillation_staged.py:369-581, :1633-1666, :1693-1719, :1351-1467)."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

MODES = ("teacher", "cached", "noteacher")
LOGIT_THRESHOLD = np.float32(1.5 * 2.0 ** -24)   # include/hiseg_metrics.h: the stated foreground predicate


def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "distill_eval.npz"))
    nb = int(z["num_batches"])
    batches = [(z[f"b{i}_student"], z[f"b{i}_teacher"], z[f"b{i}_masks"]) for i in range(nb)]
    keys = [str(k) for k in z["metric_keys"]]
    want = {m: {k: float(z[f"{m}_{k}"]) for k in keys} for m in MODES}
    loss_keys = [str(k) for k in z["loss_keys"]]
    totals = [float(z[f"b{i}_loss_total"]) for i in range(nb)]
    dicts = [{k: float(v) for k, v in zip(loss_keys, z[f"b{i}_loss_terms"])} for i in range(nb)]
    return batches, totals, dicts, want, float(z["teacher_miou_cache"])


def np_counts(student, teacher, masks):
    """numpy per-sample counts[b][4*m + 2*t + s] (the kernel's contract; teacher None: t = s).  Logits are
    compared as float32; uint8 masks are foreground when non-zero, float masks when > 0.5."""
    B = student.shape[0]
    with np.errstate(invalid="ignore"):
        s = (np.asarray(student, np.float32).reshape(B, -1) > LOGIT_THRESHOLD).astype(np.int64)
        t = s if teacher is None else (np.asarray(teacher, np.float32).reshape(B, -1) > LOGIT_THRESHOLD).astype(np.int64)
        m = (np.asarray(masks).reshape(B, -1) > 0.5).astype(np.int64)
    k = 4 * m + 2 * t + s
    return np.stack([np.bincount(row, minlength=8) for row in k]).astype(np.int64)


def mode_args(mode, cache):
    """(teacher_miou_cache, has_teacher) of a golden run."""
    return (cache if mode == "cached" else None), mode != "noteacher"


@pytest.mark.parametrize("mode", MODES)
def test_metrics_from_counts_equal_the_reference_evaluate(mode):
    from hiseg import distill_metrics_from_counts
    batches, totals, dicts, want, cache = golden()
    cache_arg, has_teacher = mode_args(mode, cache)
    counts = [np_counts(s, t if has_teacher else None, m) for s, t, m in batches]
    got = distill_metrics_from_counts(counts, totals, dicts, cache_arg, has_teacher)
    assert list(got) == list(want[mode])
    for k, w in want[mode].items():
        assert float(got[k]) == float(w), (k, float(got[k]), float(w))


def test_golden_batches_hold_the_edge_cases():
    """What the fixture is for: exact zeros, NaN and +-inf logits, masks of exactly 0.5 / 0.75 / NaN, no logit in the
    band (0, 1e-6) where the predicate is implementation-defined, and an all-background sample."""
    batches, _, _, _, _ = golden()
    s = np.concatenate([b[0].ravel() for b in batches])
    t = np.concatenate([b[1].ravel() for b in batches])
    m = np.concatenate([b[2].ravel() for b in batches])
    for x in (s, t):
        assert (x == 0).any() and np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        assert not ((x > 0) & (x < 1e-6)).any()
    assert (m == 0.5).any() and (m == 0.75).any() and np.isnan(m).any()
    c = np_counts(*batches[1])
    assert c[1, 0] == c[1].sum()     # mask, teacher and student all background


def test_metrics_from_counts_rejects_empty_and_mismatched_input():
    from hiseg import distill_metrics_from_counts
    with pytest.raises(ZeroDivisionError):
        distill_metrics_from_counts([], [], [])
    with pytest.raises(ValueError):
        distill_metrics_from_counts([np.zeros((1, 8), np.int64)], [], [])


def test_update_adaptive_distillation_follows_the_reference_glue():
    import hiseg
    loss = hiseg.UNetDistillationLoss(temperature=1.0, alpha=0.05, task_weight=0.7, adaptive_distillation=True)
    kw = dict(min_alpha=0.001, amplification_factor=20.0, zero_distillation_threshold=0.03)
    # first call: the cache is filled; the student is behind the teacher, nothing changes
    cache, msg = hiseg.update_adaptive_distillation(loss, {"student_miou": 0.70, "teacher_miou": 0.80}, None, **kw)
    assert cache == 0.80 and msg is None
    assert (loss.alpha, loss.task_weight, loss.distillation_eliminated) == (0.05, 0.7, False)
    # slightly ahead: the weights move, against the cached teacher value (the new teacher_miou is ignored)
    cache, msg = hiseg.update_adaptive_distillation(loss, {"student_miou": 0.81, "teacher_miou": 0.10}, cache, **kw)
    assert cache == 0.80 and 0.0 < loss.alpha < 0.05 and 0.7 < loss.task_weight < 1.0
    assert msg.startswith("  Adaptive distillation: Student/Teacher ratio = 1.0125") and "0.050 →" in msg
    # above teacher * (1 + threshold): eliminated for good
    cache, msg = hiseg.update_adaptive_distillation(loss, {"student_miou": 0.83, "teacher_miou": 0.80}, cache, **kw)
    assert loss.distillation_eliminated and loss.alpha == 0.0 and loss.task_weight == 1.0
    assert "PERMANENTLY ELIMINATED" in msg and "Student surpassed teacher by 3.7%" in msg
    # a later call, even with a weaker student
    cache, msg = hiseg.update_adaptive_distillation(loss, {"student_miou": 0.50, "teacher_miou": 0.80}, cache, **kw)
    assert "remains ELIMINATED" in msg and loss.alpha == 0.0 and loss.task_weight == 1.0 and cache == 0.80

    fixed = hiseg.UNetDistillationLoss(temperature=1.0, alpha=0.05, task_weight=0.7, adaptive_distillation=False)
    cache, msg = hiseg.update_adaptive_distillation(fixed, {"student_miou": 0.95, "teacher_miou": 0.80}, None, **kw)
    assert cache == 0.80 and msg is None
    assert (fixed.alpha, fixed.task_weight, fixed.distillation_eliminated, fixed.performance_ratio) == (0.05, 0.7, False, 1.0)


# ---------------------------------------------------------------------------------------------- checkpoints
REFERENCE_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "train_metrics",
                  "val_metrics", "best_iou", "config", "progressive_unfreeze_state", "loss_fn_state",
                  "teacher_miou_cache"}   # train_distillation_staged.py:1693-1719
LOSS_FIELDS = ("performance_ratio", "alpha", "task_weight", "temperature", "distillation_eliminated")


class _Wrapper(torch.nn.Module):
    """Stand-in for DistillationUNetWrapper: a student, a teacher that must not be saved, and the unfreeze hook."""

    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.student = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Conv2d(4, 1, 1))
        self.teacher = torch.nn.Conv2d(3, 1, 1)
        self.unfreeze_calls = []

    def unfreeze_encoder_blocks(self, num_blocks, learning_rate_scale=0.1):
        self.unfreeze_calls.append((num_blocks, learning_rate_scale))
        return list(self.student[0].parameters())


def _trained(seed):
    m = _Wrapper(seed)
    opt = torch.optim.AdamW(m.student.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=10)
    m.student(torch.ones(1, 3, 5, 5)).sum().backward()
    opt.step()
    sched.step()
    return m, opt, sched


def test_distillation_checkpoint_round_trip(tmp_path):
    import hiseg
    m, opt, sched = _trained(1)
    loss = hiseg.UNetDistillationLoss(temperature=3.0, alpha=0.3, task_weight=0.5)
    loss.update_temperature(3, 10, 1.0, "linear")
    loss.update_distillation_weight(0.81, 0.80, 0.0, 20.0, 0.03)   # alpha becomes a numpy float
    state = {k: getattr(loss, k) for k in LOSS_FIELDS}
    assert state["alpha"] != 0.3 and state["temperature"] != 3.0 and state["performance_ratio"] != 1.0
    path = str(tmp_path / "ck.pth")
    pu = {"enabled": True, "blocks_unfrozen": 2, "unfreeze_start_epoch": 10, "unfreeze_rate": 5, "encoder_lr_scale": 0.25}
    ck = hiseg.save_distillation_checkpoint(
        path, m, opt, 6, loss, 0.8125, best_iou=0.77, scheduler=sched, train_metrics={"total_loss": 1.5},
        val_metrics={"iou": np.float64(0.7), "student_miou": 0.7}, config={"distillation": {"alpha": 0.3}},
        progressive_unfreeze_state=pu)
    assert set(ck) == REFERENCE_KEYS
    on_disk = torch.load(path, map_location="cpu", weights_only=True)
    assert set(on_disk) == REFERENCE_KEYS
    assert set(on_disk["loss_fn_state"]) == set(LOSS_FIELDS)
    assert set(on_disk["model_state_dict"]) == set(m.student.state_dict())        # the student alone
    for k, v in m.student.state_dict().items():
        assert on_disk["model_state_dict"][k].data_ptr() != v.data_ptr() and torch.equal(on_disk["model_state_dict"][k], v)
    assert on_disk["val_metrics"] == {"iou": 0.7, "student_miou": 0.7} and on_disk["config"] == {"distillation": {"alpha": 0.3}}

    m2, opt2, sched2 = _trained(2)
    loss2 = hiseg.UNetDistillationLoss(temperature=3.0, alpha=0.3, task_weight=0.5)
    got = hiseg.resume_distillation_checkpoint(path, m2, loss2, opt2, sched2, encoder_lr_scale=0.25)
    assert got == {"start_epoch": 7, "best_iou": 0.77, "teacher_miou_cache": 0.8125, "blocks_unfrozen": 2}
    for k in LOSS_FIELDS:
        assert getattr(loss2, k) == state[k], k
    assert m2.unfreeze_calls == [(2, 0.25)]
    for k, v in m.student.state_dict().items():
        assert torch.equal(m2.student.state_dict()[k], v)
    assert not torch.equal(m2.teacher.weight, m.teacher.weight)                    # the teacher is not in the file
    p, p2 = next(m.student.parameters()), next(m2.student.parameters())
    assert torch.equal(opt2.state[p2]["exp_avg"], opt.state[p]["exp_avg"])
    assert sched2.state_dict()["last_epoch"] == sched.state_dict()["last_epoch"]


def test_distillation_checkpoint_without_adaptive_state_resumes_with_defaults(tmp_path):
    import hiseg
    m, opt, _ = _trained(3)
    loss = hiseg.UNetDistillationLoss(temperature=2.0, alpha=0.3, task_weight=0.5)
    path = str(tmp_path / "ck.pth")
    ck = hiseg.save_distillation_checkpoint(path, m, opt, 0, loss, None)
    assert ck["progressive_unfreeze_state"] is None and ck["teacher_miou_cache"] is None
    # an older checkpoint: no adaptive state at all -> the loss stays as constructed, no cache, nothing unfrozen
    old = {k: v for k, v in ck.items() if k not in ("loss_fn_state", "teacher_miou_cache", "progressive_unfreeze_state")}
    torch.save(old, path)
    m2, opt2, _ = _trained(4)
    loss2 = hiseg.UNetDistillationLoss(temperature=2.0, alpha=0.3, task_weight=0.5)
    loss2.alpha, loss2.performance_ratio = 0.2, 1.01
    got = hiseg.resume_distillation_checkpoint(path, m2, loss2, opt2)
    assert got == {"start_epoch": 1, "best_iou": 0.0, "teacher_miou_cache": None, "blocks_unfrozen": 0}
    assert (loss2.alpha, loss2.performance_ratio, loss2.task_weight, loss2.temperature) == (0.2, 1.01, 0.5, 2.0)
    assert m2.unfreeze_calls == []
    # a loss_fn_state that lacks fields: the reference's defaults (:1364-1372)
    torch.save(dict(old, loss_fn_state={"distillation_eliminated": True}), path)
    hiseg.resume_distillation_checkpoint(path, m2, loss2)
    assert (loss2.performance_ratio, loss2.alpha, loss2.task_weight, loss2.temperature,
            loss2.distillation_eliminated) == (1.0, 0.3, 0.7, 1.0, True)


def test_distillation_evaluation_refuses_cpu_tensors():
    import hiseg
    s = torch.zeros(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        hiseg.binary_seg_stats(s, s, s)
    with pytest.raises(RuntimeError, match="GPU only"):
        hiseg.binary_seg_stats(s, None, s)

    class Model(torch.nn.Module):
        teacher = None

        def forward(self, x):
            return s, s

    with pytest.raises(RuntimeError, match="GPU only"):
        hiseg.evaluate_distillation(Model(), [(s, s)], lambda a, b, c: (torch.tensor(1.0), {}), "cpu")
