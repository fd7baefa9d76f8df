"""Time the fused training augmentation (include/hiseg_augment.h) on the GPU.

    python tools/augment_bench.py [--iters 20] [--windows 7] [--out profiles/augment_bench.txt]

Workload: the training batch, 32 images of 640x640, resident on the device.  ``augment_images`` is timed for four
parameter sets applied to every sample -- identity, tables only, the HSV round trip, HSV plus a 7x7 filter -- and,
in the same run, the unchanged ``resize_bilinear_pil`` float path that it follows in GpuRoiBatchBuilder: 480x640
sources (Pillow skips the horizontal pass, so this is the vertical resample pass alone) and 375x500 sources (both
passes).  Each case is captured into a graph of ``iters`` back-to-back calls (so the host's per-call work is not
in the window) and replayed ``windows`` times between HIP events after a warm-up; the median window is reported
as time per call, GB/s over the algorithmic bytes (augment: 3 B read + 12 B written per pixel) and the share of
the HBM peak, plus each augment case's ratio to the vertical resample pass.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "human-instance-segmentation_amd"))

HBM_PEAK = 8.0e12   # bytes / s, MI355X
B, H, W = 32, 640, 640


def timed(fn, iters, windows):
    """Median over `windows` replays of a graph of `iters` calls: us per call."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: no GPU (timings are taken on the device only)")
    from hiseg.augment import (AugParams, augment_images, brightness_contrast_lut, gaussian_kernel, hsv_shift_luts)
    from hiseg.data import resize_bilinear_pil
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    bc, hsv, k7 = brightness_contrast_lut(1.1, -0.05), hsv_shift_luts(7, -12, 9), gaussian_kernel(7, 2.0)
    cases = {"identity": {}, "tables only": dict(rgb_lut=bc), "HSV": dict(hsv_luts=hsv, rgb_lut=bc),
             "HSV + 7x7": dict(hsv_luts=hsv, rgb_lut=bc, kernel=k7)}
    lines = [f"device {torch.cuda.get_device_name(0)}; graph of {args.iters} calls, {args.windows} replays, median "
             f"(min .. max) per call; HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s",
             f"== {B} x {H}x{W}, resident inputs =="]
    rows = []
    for name, src_hw in (("resize_bilinear_pil f32, 480x640 sources (vertical pass alone)", (480, 640)),
                         ("resize_bilinear_pil f32, 375x500 sources (both passes)", (375, 500))):
        src = torch.randint(0, 256, (B, *src_hw, 3), dtype=torch.uint8, device=dev, generator=gen)
        t = timed(lambda: resize_bilinear_pil(src, (W, H)), args.iters, args.windows)
        rows.append((name, t, B * (src_hw[0] * src_hw[1] * 3 + H * W * 12)))
    t_v = rows[0][1][0]
    for name, kw in cases.items():
        p = AugParams(B)
        for i in range(B):
            p.set(i, flip=bool(i & 1), **kw)
        p.to(dev)
        t = timed(lambda: augment_images(imgs, p, out=out), args.iters, args.windows)
        rows.append((f"augment_images, {name} (odd samples flipped)", t, B * H * W * 15))
    for name, (med, lo, hi), nbytes in rows:
        gbs = nbytes / (med * 1e-6) / 1e9
        lines.append(f"  {name:<66s} {med:8.1f} us ({lo:7.1f} .. {hi:7.1f})  {nbytes / 1e6:7.1f} MB  {gbs:7.0f} GB/s  "
                     f"{100 * gbs * 1e9 / HBM_PEAK:5.1f}% of HBM peak  {med / t_v:5.2f}x the vertical pass")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
