"""Distillation validation on the GPU (hiseg.distill_eval over hiseg_binary_seg_stats, include/hiseg_metrics.h):
the histogram kernel against exact host counts, evaluate_distillation against the reference's own evaluate
(tests/golden/distill_eval.npz) and, on the real student / teacher modules and loss, against itself."""
import numpy as np
import pytest
import torch

from test_distill_eval import MODES, golden, mode_args, np_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, H, W): scalar path (HW % 4 != 0); one pixel; vector path; one 4-pixel group past a block's 4096-pixel span;
# many blocks per sample (the atomics)
SHAPES = [(3, 7, 5), (2, 1, 1), (4, 16, 12), (2, 41, 100), (2, 640, 640)]


def _inputs(shape, seed):
    """Seeded logits (with exact zeros and values that bf16 rounding moves) and masks: float32 blobs and uint8 with
    0, 1 and 255."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((B, 1, H, W)) * 2).astype(np.float32)
    t = (rng.standard_normal((B, 1, H, W)) * 2).astype(np.float32)
    s[rng.random(s.shape) < 0.1] = 0.0
    t[rng.random(t.shape) < 0.1] = 0.0
    mf = rng.random((B, 1, H, W)).astype(np.float32)
    mu = rng.choice(np.array([0, 0, 1, 255], np.uint8), size=(B, 1, H, W))
    return s, t, mf, mu


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_kernel_matches_host_counts(shape):
    from hiseg import binary_seg_stats
    s, t, mf, mu = _inputs(shape, sum(shape))
    ts, tt = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    bs, bt = ts.bfloat16(), tt.bfloat16()
    ws, wt = bs.float().cpu().numpy(), bt.float().cpu().numpy()          # the widened bf16 values
    for mask in (mf, mu):
        tm = torch.from_numpy(mask).to(DEV)
        for (a, b, na, nb) in ((ts, tt, s, t), (bs, bt, ws, wt), (ts, bt, s, wt)):
            got = binary_seg_stats(a, b, tm)
            assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0], 8)
            np.testing.assert_array_equal(got.cpu().numpy(), np_counts(na, nb, mask), err_msg=str((a.dtype, b.dtype, mask.dtype)))
            got = binary_seg_stats(a, None, tm)
            np.testing.assert_array_equal(got.cpu().numpy(), np_counts(na, None, mask), err_msg=str((a.dtype, mask.dtype)))
    # every pixel is counted once
    assert int(binary_seg_stats(ts, tt, torch.from_numpy(mf).to(DEV)).sum()) == s.size


def test_stats_kernel_special_values():
    """The stated predicate: 0.0, -0.0, NaN, -inf, negatives and 2^-24 are background; 2^-23, 1e-6 and +inf are
    foreground.  Masks: 0.5 and NaN are background, 0.75 foreground.  Scalar and vector paths."""
    from hiseg import binary_seg_stats
    nan, inf = float("nan"), float("inf")
    logits = [0.0, -0.0, nan, inf, -inf, 2.0 ** -24, 2.0 ** -23, 1e-6, -1e-6, 0.25, -0.25, 3.0]
    bits = [0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1]
    masks = [0.5, nan, 0.75, 1.0, 0.0, 0.5 + 2.0 ** -24, 0.25, inf, -inf, 0.5, nan, 0.75]
    mbits = [0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 0, 1]
    for n in (12, 11):                                   # HW = 12: vector path; 11: scalar path
        s = torch.tensor(logits[:n], device=DEV).view(1, 1, 1, n)
        t = torch.tensor(logits[:n][::-1], device=DEV).view(1, 1, 1, n)
        m = torch.tensor(masks[:n], device=DEV).view(1, 1, 1, n)
        want = np.zeros((1, 8), np.int64)
        for sb, tb, mb in zip(bits[:n], bits[:n][::-1], mbits[:n]):
            want[0, 4 * mb + 2 * tb + sb] += 1
        np.testing.assert_array_equal(binary_seg_stats(s, t, m).cpu().numpy(), want)
        np.testing.assert_array_equal(np_counts(s.cpu().numpy(), t.cpu().numpy(), m.cpu().numpy()), want)


def test_stats_kernel_misaligned_views_out_accumulation_and_errors():
    from hiseg import binary_seg_stats
    g = torch.Generator(device=DEV).manual_seed(9)
    n = 2 * 8 * 8
    base = [torch.randn(n + 1, device=DEV, generator=g) for _ in range(3)]
    s, t, m = (b[1:].view(2, 1, 8, 8) for b in base)    # storage offset of one element: the scalar path
    want = binary_seg_stats(s.clone(), t.clone(), m.clone())
    assert torch.equal(binary_seg_stats(s, t, m), want)
    assert torch.equal(binary_seg_stats(s.clone(), t, m.clone()), want)
    mu = (torch.rand(n + 1, device=DEV, generator=g) < 0.5).to(torch.uint8)[1:].view(2, 1, 8, 8)
    assert torch.equal(binary_seg_stats(s.clone(), None, mu), binary_seg_stats(s.clone(), None, mu.clone()))
    assert torch.equal(binary_seg_stats(s, None, mu.bool()), binary_seg_stats(s, None, mu))
    # out= accumulates
    s2 = torch.randn(2, 1, 8, 8, device=DEV, generator=g)
    out = binary_seg_stats(s, t, m)
    assert binary_seg_stats(s2, t, m, out=out) is out
    assert torch.equal(out, want + binary_seg_stats(s2, t, m))
    with pytest.raises(ValueError):
        binary_seg_stats(s, t[:1], m)
    with pytest.raises(ValueError):
        binary_seg_stats(s, t, m[:, :, :4])
    with pytest.raises(ValueError):
        binary_seg_stats(s, t, m, out=torch.zeros(2, 4, dtype=torch.int64, device=DEV))


class _Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars[tag] = (value, step)


@pytest.mark.parametrize("mode", MODES)
def test_evaluate_distillation_matches_reference_golden(mode):
    """The reference's evaluate run on recorded logits / loss values; here the same batches through
    hiseg.evaluate_distillation (device logits, device loss totals, one histogram launch per batch)."""
    import hiseg
    batches, totals, dicts, want, cache = golden()
    cache_arg, has_teacher = mode_args(mode, cache)

    class Replay(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.teacher = torch.nn.Identity() if has_teacher else None
            self.k = 0

        def forward(self, images):
            s, t, _ = batches[self.k]
            self.k += 1
            s = torch.from_numpy(s).to(DEV)
            return s, (torch.from_numpy(t).to(DEV) if has_teacher else torch.zeros_like(s))

    class ReplayLoss:
        k = 0

        def __call__(self, student, teacher, masks):
            i = self.k
            self.k += 1
            return torch.tensor(totals[i], device=DEV), dict(dicts[i])

    loader = [(torch.zeros(m.shape[0], 3, 8, 8), torch.from_numpy(m)) for _, _, m in batches]
    writer = _Writer()
    model = Replay().train()
    got = hiseg.evaluate_distillation(model, loader, ReplayLoss(), DEV, 4, writer, teacher_miou_cache=cache_arg)
    assert not model.training
    assert list(got) == list(want[mode])
    for k, w in want[mode].items():
        assert float(got[k]) == float(w), (k, float(got[k]), float(w))
    tags = {"Val/Loss": "total_loss", "Val/KL_Loss": "kl_loss", "Val/MSE_Loss": "mse_loss", "Val/BCE_Loss": "bce_loss",
            "Val/Dice_Loss": "dice_loss", "Val/Student_mIoU": "student_miou", "Val/Teacher_mIoU": "teacher_miou",
            "Val/Agreement": "agreement", "Val/mIoU_Diff": "miou_diff"}
    assert writer.scalars == {tag: (want[mode][k], 4) for tag, k in tags.items()}


def test_evaluate_distillation_empty_loader_and_visualize_warning():
    import hiseg
    model = torch.nn.Identity()
    model.teacher = None
    with pytest.raises(ZeroDivisionError):
        hiseg.evaluate_distillation(model, [], None, DEV)
    with pytest.warns(UserWarning, match="visualisation panels"), pytest.raises(ZeroDivisionError):
        hiseg.evaluate_distillation(model, [], None, DEV, visualize_dir="somewhere")


def test_evaluate_distillation_with_the_hip_models_and_loss():
    """B0 student + B0 teacher (random weights) and the real UNetDistillationLoss: the metrics equal
    distill_metrics_from_counts on counts taken with torch ops from the logits the same model returns for the same
    inputs, and the loss averages equal the means of separate loss calls.  Self-consistency, not a comparison with
    the CPU: logits near zero may legitimately differ between the two."""
    import filler
    import hiseg
    model, loss_fn = hiseg.create_unet_distillation_model("timm-efficientnet-b0", "timm-efficientnet-b0",
                                                          teacher_checkpoint="absent.pth", device="cpu")
    assert model.teacher is not None
    filler.fill_module(model.student, seed=11)
    filler.fill_module(model.teacher, seed=12)
    model = model.to(DEV)
    loader = []
    for k in range(2):
        images = torch.from_numpy(filler.normal(700 + k, (2, 3, 64, 64)))
        yy, xx = np.mgrid[0:64, 0:64]
        masks = np.stack([((yy - 30 - 4 * i) ** 2 + (xx - 28 + 6 * k) ** 2 < (14 + 3 * i) ** 2) for i in range(2)])
        loader.append((images, torch.from_numpy(masks[:, None].astype(np.float32))))
    got = hiseg.evaluate_distillation(model, loader, loss_fn, DEV)

    loss2 = hiseg.UNetDistillationLoss(temperature=1.0, alpha=0.05, task_weight=0.7, use_dice_loss=True)
    counts, totals, dicts = [], [], []
    with torch.no_grad():
        for images, masks in loader:
            s, t = model(images.to(DEV))
            for x in (s, t):       # the predicate is stated outside this band only
                assert not ((x > 0) & (x < 1e-6)).any()
            sb, tb = (torch.sigmoid(x.float()) > 0.5 for x in (s, t))
            mb = masks.to(DEV) > 0.5
            idx = (4 * mb.long() + 2 * tb.long() + sb.long()).view(2, -1)
            counts.append(torch.stack([torch.bincount(r, minlength=8) for r in idx]).cpu())
            loss, d = loss2(s, t, masks.to(DEV))
            totals.append(loss.item())
            dicts.append({k: d[k] for k in ("kl_loss", "mse_loss", "bce_loss", "dice_loss")})
    want = hiseg.distill_metrics_from_counts(counts, totals, dicts)
    assert got == want
    assert got["total_loss"] == sum(totals) / 2 and got["bce_loss"] == sum(d["bce_loss"] for d in dicts) / 2
    assert 0.0 < got["student_miou"] < 1.0 and 0.0 < got["agreement"] <= 1.0
