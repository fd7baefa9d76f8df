"""Time the full-frame instance composition (include/hiseg_compose.h) on the GPU.

    python tools/compose_bench.py [--iters 50] [--windows 5] [--out profiles/compose_bench.txt]

Two shapes: the C2 serving shape (256 masks of 128x96 into 32 frames of 480x640, 8 overlapping ROIs per frame) and one
1080x1920 frame with 32 ROIs.  Per shape:
  * hiseg: classify, compose and overlay, each timed alone with HIP events over windows of calls after a warm-up
    (median window), with the fraction of the HBM peak its algorithmic bytes amount to;
  * torch: the same label map from torch-ROCm ops on the device, one F.interpolate(mode='nearest') and one masked
    assignment per ROI (box arithmetic done on the host beforehand, outside the timed region; F.interpolate's nearest
    map is not cv2's, so this is a cost comparison, not a parity check);
  * host: the reference's loop restated in numpy (softmax / argmax / threshold, nearest resize, paste, np.where paint,
    blend) for ONE frame's worth of ROIs on the CPU.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "human-instance-segmentation_amd"))

HBM_PEAK = 8.0e12   # bytes / s, MI355X


def make(B, H, W, per_frame, mh, mw, dev):
    g = torch.Generator().manual_seed(7)
    N = B * per_frame
    yy, xx = torch.meshgrid(torch.arange(mh), torch.arange(mw), indexing="ij")
    inside = (((yy - mh / 2) / (0.4 * mh)) ** 2 + ((xx - mw / 2) / (0.4 * mw)) ** 2 < 1).float()
    logits = torch.randn(N, 3, mh, mw, generator=g)
    logits[:, 1] += inside * 4 - 1
    rois = torch.zeros(N, 5)
    rois[:, 0] = torch.arange(N) // per_frame
    cx, cy = 0.3 + 0.4 * torch.rand(N, generator=g), 0.3 + 0.4 * torch.rand(N, generator=g)   # overlapping boxes
    bw, bh = 0.15 + 0.2 * torch.rand(N, generator=g), 0.3 + 0.3 * torch.rand(N, generator=g)
    rois[:, 1], rois[:, 2] = (cx - bw / 2).clamp(0, 1), (cy - bh / 2).clamp(0, 1)
    rois[:, 3], rois[:, 4] = (cx + bw / 2).clamp(0, 1), (cy + bh / 2).clamp(0, 1)
    image = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    return logits.to(dev), rois.to(dev), image.to(dev)


def timed(fn, iters, windows):
    """Median over `windows` of the mean time per call (us) of `iters` back-to-back calls."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(out))


def torch_compose(masks, boxes, B, H, W):
    """Label map from torch ops: per ROI one nearest resize and one masked assignment (later ROI wins)."""
    label = torch.zeros(B, H, W, dtype=torch.int32, device=masks.device)
    for k, (b, x1, y1, x2, y2) in enumerate(boxes):
        if x2 <= x1 or y2 <= y1:
            continue
        m = F.interpolate(masks[k:k + 1], size=(y2 - y1, x2 - x1), mode="nearest")[0, 0] > 0.5
        label[b, y1:y2, x1:x2].masked_fill_(m, k + 1)
    return label


def host_frame(logits, rois, image, colors, H, W, thr, alpha):
    """The reference's consumer for one frame in numpy (test_hierarchical_instance_peopleseg_onnx.py:230-291, 336-402)."""
    overlay = np.zeros_like(image)
    for k in range(len(rois)):
        l = logits[k]
        e = np.exp(l - l.max(0, keepdims=True))
        p = e / e.sum(0, keepdims=True)
        target = (p.argmax(0) == 1) & (p.max(0) > thr)
        x1, y1, x2, y2 = int(rois[k, 1] * W), int(rois[k, 2] * H), int(rois[k, 3] * W), int(rois[k, 4] * H)
        if x2 <= x1 or y2 <= y1 or not target.any():
            continue
        mh, mw = target.shape
        xs = np.minimum(np.floor(np.arange(x2 - x1) * (1.0 / ((x2 - x1) / float(mw)))).astype(np.int64), mw - 1)
        ys = np.minimum(np.floor(np.arange(y2 - y1) * (1.0 / ((y2 - y1) / float(mh)))).astype(np.int64), mh - 1)
        full = np.zeros((H, W), np.uint8)
        full[y1:y2, x1:x2] = target[ys][:, xs]
        colored = np.zeros_like(overlay)
        colored[full > 0] = colors[k]
        overlay = np.where(np.stack([full] * 3, axis=-1) > 0, colored, overlay)
    t = image.astype(np.float32) * np.float32(1 - alpha) + overlay.astype(np.float32) * np.float32(alpha)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import hiseg
    from hiseg import ops
    dev = "cuda:0"
    lines = [f"device {torch.cuda.get_device_name(0)}; {a.windows} windows of {a.iters} calls, median window; "
             f"HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s"]
    for name, (B, H, W, per) in (("C2 32x480x640, 8 ROIs/frame", (32, 480, 640, 8)),
                                 ("1x1080x1920, 32 ROIs", (1, 1080, 1920, 32))):
        mh, mw = 128, 96
        logits, rois, image = make(B, H, W, per, mh, mw, dev)
        N = logits.shape[0]
        colors = hiseg.instance_colors(N).to(dev)
        bits, score, _ = ops.roi_mask_classify(logits, 0.5)
        label = ops.compose_instance_map(bits, score, rois, (B, H, W), mw)
        masks = ops.instance_masks(logits)
        r = rois.cpu().numpy()
        boxes = [(int(v[0]), int(v[1] * np.float32(W)), int(v[2] * np.float32(H)), int(v[3] * np.float32(W)),
                  int(v[4] * np.float32(H))) for v in r]
        px, nbits = B * H * W, bits.numel() * 4
        rows = [("hiseg classify", lambda: ops.roi_mask_classify(logits, 0.5), logits.numel() * 4 + nbits + 8 * N),
                ("hiseg pack", lambda: ops.roi_mask_pack(masks), masks.numel() * 4 + nbits + 8 * N),
                ("hiseg compose", lambda: ops.compose_instance_map(bits, score, rois, (B, H, W), mw),
                 px * 4 + nbits + 24 * N),
                ("hiseg overlay", lambda: ops.instance_overlay(label, image, colors, 0.5), px * (4 + 3 + 3)),
                ("torch compose (interpolate + masked assign per ROI)", lambda: torch_compose(masks, boxes, B, H, W),
                 None)]
        lines.append(f"== {name}: N = {N}, masks {mh}x{mw}, painted {float((label > 0).float().mean()) * 100:.1f}% ==")
        res = {}
        for what, fn, nbytes in rows:
            us = res[what] = timed(fn, a.iters if nbytes else max(a.iters // 10, 3), a.windows)
            frac = f"  {nbytes / 1e6:8.2f} MB  {nbytes / (us * 1e-6) / HBM_PEAK * 100:5.1f}% of HBM peak" if nbytes else ""
            lines.append(f"  {what:<54s} {us:10.1f} us{frac}")
        lines.append(f"  hiseg compose vs torch compose: {res[rows[4][0]] / res['hiseg compose']:.1f}x faster")
        k = slice(0, per)
        hl, hr, hi, hc = (logits[k].cpu().numpy(), r[k], image[0].cpu().numpy(), colors[k].cpu().numpy())
        t0 = time.perf_counter()
        for _ in range(3):
            host_frame(hl, hr, hi, hc, H, W, 0.5, 0.5)
        dt = (time.perf_counter() - t0) / 3
        lines.append(f"  host loop (numpy, one frame, {per} ROIs)                 {dt * 1e6:10.1f} us  "
                     f"(x {B} frames = {dt * B * 1e3:.1f} ms per step)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
