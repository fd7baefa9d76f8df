"""Time the plain RGB model (HierarchicalRGBSegmentationModel) and the any-size combine kernel on the GPU.

    python tools/rgb_plain_bench.py [--configs r64m64,r80m112,r112m160] [--images 32] [--rois 8] [--iters 10]
                                    [--windows 5] [--out profiles/rgb_plain_bench.txt]

Workload: the reference's `rgb_hierarchical_unet_v2_attention_<config>` experiment configs (plain model, attention
modules, layernorm2d, no refinement flag), bf16 compute, `--images` frames of 640x640 with `--rois` ROIs each, inputs
resident on the device.  Per config the model is built through the factory, loads a reference-format checkpoint
strictly, and runs `model.infer`:
  * ROI masks / s of `infer`: device events around `--iters` back-to-back calls after a warm-up, the median of
    `--windows` windows (and their min-max);
  * hiseg_hier_combine_resize on its own, on the shapes the model sends it (nothing when mask = 2 x ROI: the model then
    launches hiseg_hier_combine): time per launch from device events around back-to-back launches (the launches queue
    behind each other, so this is the kernel's time plus the gap between two launches, not a profiler's figure), and
    the bytes it must move over that time -- it reads `low` (8 B per ROI pixel) and the two target logits at 2 x ROI
    (8 B per pixel), and writes 3 floats per mask pixel, 7 with the aux outputs -- beside the HBM peak.
There is no pass / fail number: these are first measurements.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "human-instance-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

HBM_PEAK = 8.0e12   # bytes / s, MI355X
CONFIGS = {"r28m56": (28, 56), "r64m64": (64, 64), "r64m96": (64, 96), "r80m112": (80, 112), "r80m160": (80, 160),
           "r96m160": (96, 160), "r112m160": (112, 160), "r112m224": (112, 224)}


def timed(fn, iters, windows):
    """Per-call times (us) of `windows` windows of `iters` back-to-back calls: (median, min, max)."""
    for _ in range(3):
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
    return float(np.median(out)), min(out), max(out)


def combine_bytes(N, h, w, mh, mw, aux):
    return N * (h * w * 8 + 4 * h * w * 8 + mh * mw * 4 * (7 if aux else 3))


def build(roi, mask, dev):
    """The factory's plain model with a reference-format checkpoint loaded strictly, bf16."""
    import filler
    import hiseg
    kw = dict(roi_size=roi, mask_size=mask, use_attention_module=True)
    src = filler.fill_module(hiseg.create_rgb_hierarchical_model(**kw))
    model = hiseg.create_rgb_hierarchical_model(**kw)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "plain.pth")
        torch.save({"model_state_dict": src.state_dict(), "epoch": 0}, path)
        model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True)["model_state_dict"], strict=True)
    assert type(model) is hiseg.HierarchicalRGBSegmentationModel
    return hiseg.set_compute_dtype(model.eval().to(dev), torch.bfloat16)


def kernel_alone(N, h, w, mh, mw, aux, dev, iters, windows):
    from hiseg import _lib as L, ops
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)   # noqa: E731
    low, tn2 = r(N, h, w, 2), r(N * 4 * h * w, 2)
    ut_w, sc, sh, u1_w, u1_b = r(2, 32, 2, 2) * 0.5, 1 + 0.1 * r(N, 32), 0.1 * r(N, 32), r(2, 32) * 0.3, r(2) * 0.1
    fn = lambda: ops.hier_combine_resize(low, N, h, w, tn2, ut_w, sc, sh, L.ACT_RELU, u1_w, u1_b, mh, mw, aux,   # noqa: E731
                                         per_sample=True)
    return timed(fn, iters, windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="r64m64,r80m112,r112m160")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--rois", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rgb_plain_bench: no GPU (nothing is measured on the CPU)")
    import filler
    dev = torch.device("cuda:0")
    B, N = args.images, args.images * args.rois
    images = torch.from_numpy(filler.uniform(81, (B, 3, 640, 640))).to(dev)
    rois = torch.from_numpy(filler.box_rois(82, B, args.rois)).to(dev)
    lines = [f"plain RGB model, bf16, {B} images of 640x640, {args.rois} ROIs each ({N} ROI masks per call), "
             f"{torch.cuda.get_device_name(0)}; windows of {args.iters} calls, median (min-max) of {args.windows}"]
    for name in args.configs.split(","):
        roi, mask = CONFIGS[name]
        model = build(roi, mask, dev)
        with torch.no_grad():
            logits = model.infer(images, rois)
            torch.cuda.synchronize()
            assert tuple(logits.shape) == (N, 3, mask, mask) and bool(torch.isfinite(logits).all())
            med, lo, hi = timed(lambda: model.infer(images, rois), args.iters, args.windows)
        lines.append(f"{name}: infer {med / 1e3:.2f} ms / call ({lo / 1e3:.2f}-{hi / 1e3:.2f}), "
                     f"{N / med * 1e6:.0f} ROI masks / s")
        if mask != 2 * roi:
            for aux in (False, True):
                k, klo, khi = kernel_alone(N, roi, roi, mask, mask, aux, dev, 10 * args.iters, args.windows)
                nbytes = combine_bytes(N, roi, roi, mask, mask, aux)
                lines.append(f"  hier_combine_resize {roi}x{roi} -> {mask}x{mask}{' +aux' if aux else ''}: "
                             f"{k:.1f} us / launch ({klo:.1f}-{khi:.1f}), {nbytes / 1e6:.1f} MB to move, "
                             f"{nbytes / k * 1e6 / 1e12:.2f} TB/s ({100 * nbytes / k * 1e6 / HBM_PEAK:.0f} % of the "
                             f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak)")
        else:
            lines.append("  mask = 2 x ROI: hiseg_hier_combine, the new kernel is not launched")
        del model
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
