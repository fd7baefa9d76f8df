"""Time the distillation-validation histogram (hiseg.binary_seg_stats, include/hiseg_metrics.h) on the GPU.

    python tools/distill_eval_bench.py [--iters 50] [--windows 5] [--out profiles/distill_eval_bench.txt]

One shape: a validation batch of 8 x 1 x 640 x 640 float32 student logits, teacher logits and masks.
  * hiseg: one binary_seg_stats launch (12 bytes per pixel read once), timed with HIP events over windows of calls
    after a warm-up (median window), with the fraction of the HBM peak those bytes amount to;
  * torch: the reference's per-batch metric code (train_distillation_staged.py:444-492: sigmoid / threshold, the
    twelve masked products and sums, the IoU ratios, the agreement) restated with torch ops on the same device, once
    with the reference's three ``.item()`` synchronisations and once with the three values left on the device.
Both rotate over 8 input sets (315 MB, more than the 256 MiB last-level cache), so that every call streams from HBM
and not from a cache an earlier call filled.  The two sides are checked against each other before timing.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "human-instance-segmentation_amd"))

HBM_PEAK = 8.0e12   # bytes / s, MI355X
SETS = 8


def make(B, H, W, dev, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    r = torch.rand(B, 2, generator=g) * 0.4 + 0.3
    m = ((yy[None] / r[:, 0, None, None]) ** 2 + (xx[None] / r[:, 1, None, None]) ** 2 < 1).float()[:, None]
    # quantised to 1/64: no logit in (0, 1e-6), where the stated predicate and torch's sigmoid may differ
    s = torch.round((torch.randn(B, 1, H, W, generator=g) * 2 + (m - 0.5) * 2) * 64) / 64
    t = torch.round((torch.randn(B, 1, H, W, generator=g) + (m - 0.5) * 4) * 64) / 64
    return s.to(dev), t.to(dev), m.to(dev)


def torch_chain(student_output, teacher_output, masks, sync):
    """train_distillation_staged.py:444-492 (with a teacher, no cached teacher mIoU)."""
    student_preds = (torch.sigmoid(student_output) > 0.5).float()
    teacher_preds = (torch.sigmoid(teacher_output) > 0.5).float()
    masks_binary = (masks > 0.5).float()
    out = []
    for preds in (student_preds, teacher_preds):
        bg_tp = ((1 - preds) * (1 - masks_binary)).sum(dim=(1, 2, 3))
        bg_fp = ((1 - preds) * masks_binary).sum(dim=(1, 2, 3))
        bg_fn = (preds * (1 - masks_binary)).sum(dim=(1, 2, 3))
        bg_iou = bg_tp / (bg_tp + bg_fp + bg_fn + 1e-6)
        fg_tp = (preds * masks_binary).sum(dim=(1, 2, 3))
        fg_fp = (preds * (1 - masks_binary)).sum(dim=(1, 2, 3))
        fg_fn = ((1 - preds) * masks_binary).sum(dim=(1, 2, 3))
        fg_iou = fg_tp / (fg_tp + fg_fp + fg_fn + 1e-6)
        miou = ((bg_iou + fg_iou) / 2.0).mean()
        out.append(miou.item() if sync else miou)
    agreement = (student_preds == teacher_preds).float().mean(dim=(1, 2, 3)).mean()
    out.append(agreement.item() if sync else agreement)
    return out


def timed(fn, iters, windows):
    """Median over `windows` of the mean time per call (us) of `iters` back-to-back calls; fn(i) takes the call index."""
    for i in range(2 * SETS):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_eval_bench: no GPU (timings are taken on the device only)")
    import hiseg
    dev = "cuda:0"
    B, H, W = 8, 640, 640
    sets = [make(B, H, W, dev, 100 + k) for k in range(SETS)]
    nbytes = B * H * W * 12
    # the two sides agree on the data they are timed on
    for s, t, m in sets[:2]:
        counts = [hiseg.binary_seg_stats(s, t, m).cpu()]
        got = hiseg.distill_metrics_from_counts(counts, [0.0], [{}])
        want = torch_chain(s, t, m, True)
        # same counts; the device's float32 means may reduce in another order than the host's
        assert np.allclose([got["student_miou"], got["teacher_miou"], got["agreement"]], want, rtol=0, atol=1e-6), \
            (got, want)
    out = torch.zeros(B, 8, dtype=torch.int64, device=dev)
    rows = [("hiseg binary_seg_stats (one launch)", lambda i: hiseg.binary_seg_stats(*sets[i % SETS])),
            ("hiseg binary_seg_stats (out= given, no allocation)",
             lambda i: hiseg.binary_seg_stats(*sets[i % SETS], out=out)),
            ("torch chain :444-492, values left on the device", lambda i: torch_chain(*sets[i % SETS], False)),
            ("torch chain :444-492, three .item() as the reference", lambda i: torch_chain(*sets[i % SETS], True))]
    lines = [f"device {torch.cuda.get_device_name(0)}; {B}x1x{H}x{W} float32 student, teacher, mask; {a.windows} windows "
             f"of {a.iters} calls over {SETS} rotating input sets, median window; HBM peak taken as "
             f"{HBM_PEAK / 1e12:.1f} TB/s"]
    res = {}
    for what, fn in rows:
        us = res[what] = timed(fn, a.iters, a.windows)
        frac = (f"  {nbytes / 1e6:6.2f} MB  {nbytes / (us * 1e-6) / 1e12:5.2f} TB/s  "
                f"{nbytes / (us * 1e-6) / HBM_PEAK * 100:5.1f}% of HBM peak") if what.startswith("hiseg") else ""
        lines.append(f"  {what:<56s} {us:10.1f} us{frac}")
    k = res[rows[0][0]]
    lines.append(f"  torch chain vs hiseg: {res[rows[2][0]] / k:.1f}x (on device), {res[rows[3][0]] / k:.1f}x (with .item())")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
