"""UNet-guided head benchmark (developer tool, GPU): the export contract of the guided-head model against the refined
B0 model on the C2 workload shape -- 32 images of 480x640, 8 ROIs each, ROI 64x48, mask 128x96, bf16 -- and the three
kernels of include/hiseg_guided_head.h alone at that shape.

Contract rows: ROI masks per second of RGBHierarchicalExportWrapper (full-image UNet included), from HIP events
around windows of CALLS calls; the two models alternate window by window in the same process, WARMUP untimed calls
each, the median of REPEATS windows.  The ratio guided / refined is the figure to read; no target is fixed.

Kernel rows: us per call from HIP events around CALLS back-to-back launches of one entry point (launch gaps and the
Python wrapper included: a call time, an upper bound of the kernel time), the bytes the kernel has to move by
construction (computed from the shapes below) and the bytes / s that gives against the 8.0 TB/s HBM peak.

Prints one JSON object; --markdown adds the tables for DESIGN.md.  A run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "human-instance-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import filler  # noqa: E402
import hiseg  # noqa: E402
from hiseg import ops  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s
WARMUP, REPEATS, CALLS = 3, 7, 5
B, PER, IMG, ROI, MASK = 32, 8, (480, 640), (64, 48), (128, 96)
KW = dict(roi_size=ROI, mask_size=MASK, use_attention_module=True, normalization_type="batchnorm",
          activation_function="relu", use_pretrained_unet=True, pretrained_weights_path="",
          freeze_pretrained_weights=True, use_full_image_unet=True, encoder_name="timm-efficientnet-b0",
          hierarchical_base_channels=64, hierarchical_depth=3)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls   # us per call


def alternate(fns, calls=CALLS):
    """Median / min / max us per call of each fn, the fns taking turns window by window."""
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(REPEATS):
        for i, fn in enumerate(fns):
            us[i].append(window(fn, calls))
    return [(statistics.median(u), min(u), max(u)) for u in us]


def contract_rows():
    images = torch.from_numpy(filler.uniform(1, (B, 3) + IMG)).cuda()
    rois = torch.from_numpy(filler.box_rois(2, B, PER)).cuda()
    wraps = []
    for name, flags in (("guided head", {}), ("refined B0 head", dict(use_contour_detection=True,
                                                                       use_distance_transform=True))):
        m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**KW, **flags))
        m = hiseg.set_compute_dtype(m, torch.bfloat16).cuda().eval()
        wraps.append((name, hiseg.RGBHierarchicalExportWrapper(m)))
    with torch.no_grad():
        t = alternate([lambda w=w: w(images, rois) for _, w in wraps])
    rows = [{"row": f"export contract, {name}", "us": med, "us_min": lo, "us_max": hi,
             "roi_masks_per_s": B * PER / (med * 1e-6)} for (name, _), (med, lo, hi) in zip(wraps, t)]
    return rows, rows[0]["roi_masks_per_s"] / rows[1]["roi_masks_per_s"]


def kernel_rows():
    N, (h, w), (mh, mw) = B * PER, ROI, MASK
    P, dev, bf = N * h * w, "cuda", torch.bfloat16
    mask = torch.from_numpy(filler.normal(3, (N, 2, h, w)) * 3.0).to(dev)
    y = ops.Act.from_nchw(torch.from_numpy(filler.normal(4, (N, 256, h, w))).to(dev), bf)
    z = ops.Act.from_nchw(torch.from_numpy(filler.normal(5, (N, 128, h, w))).to(dev), bf)
    w1 = torch.from_numpy(filler.normal(6, (64, 256, 1, 1)) / 16).to(dev)
    b1, w2, b2 = (torch.from_numpy(filler.normal(s, shp) * 0.1).to(dev) for s, shp in ((7, (64,)), (8, (64,)), (9, (1,))))
    w3, b3 = torch.from_numpy(filler.normal(10, (3, 128)) / 11).to(dev), torch.zeros(3, device=dev)
    w1t, frag = ops.pack_guided_attn(w1, bf, dev)
    _, _, factor = ops.guided_prep(mask, bf, want_factor=True)
    halo = 10 / 8   # source rows the finish kernel reads per 8 it owns (x2 resize, 16 output rows per workgroup)
    cases = [
        ("guided_prep (fg_prob chunk + factor)", lambda: ops.guided_prep(mask, bf, want_factor=True), P * (4 + 16 + 4)),
        ("guided_attn, matrix-core form", lambda: ops.guided_attn(y, w1t, b1, w2, b2, 1, factor, w1_frag=frag),
         P * (512 + 4 + 4)),
        ("guided_attn, one thread per pixel", lambda: ops.guided_attn(y, w1t, b1, w2, b2, 1, factor), P * (512 + 4 + 4)),
        ("guided_finish, aux none", lambda: ops.guided_finish(z, w3, b3, mh, mw), int(P * 256 * halo) + 4 * P * 12),
        ("guided_finish, aux full", lambda: ops.guided_finish(z, w3, b3, mh, mw, mask=mask, want_aux=True),
         int(P * (256 + 4) * halo) + 4 * P * (12 + 8 + 8 + 4 + 4)),
    ]
    t = alternate([fn for _, fn, _ in cases], calls=20)
    return [{"row": name, "us": med, "us_min": lo, "us_max": hi, "bytes": nbytes,
             "bytes_per_s": nbytes / (med * 1e-6), "hbm_frac": nbytes / (med * 1e-6) / HBM_PEAK}
            for (name, _, nbytes), (med, lo, hi) in zip(cases, t)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guided_head_bench: no GPU (the tool measures on the device; there is no CPU fall-back)")
    crow, ratio = contract_rows()
    krow = kernel_rows()
    print(json.dumps({"workload": {"images": B, "rois": B * PER, "image": IMG, "roi": ROI, "mask": MASK},
                      "contract": crow, "guided_over_refined": ratio, "kernels": krow}))
    if args.markdown:
        print("| row | us / call (min-max) | ROI masks / s |\n|---|---|---|")
        for r in crow:
            print(f"| {r['row']} | {r['us']:.0f} ({r['us_min']:.0f}-{r['us_max']:.0f}) | {r['roi_masks_per_s']:.0f} |")
        print(f"\nguided / refined: {ratio:.2f}x\n")
        print("| kernel | us / call (min-max) | MB by construction | TB/s | of 8.0 TB/s |\n|---|---|---|---|---|")
        for r in krow:
            print(f"| {r['row']} | {r['us']:.1f} ({r['us_min']:.1f}-{r['us_max']:.1f}) | {r['bytes'] / 1e6:.0f} | "
                  f"{r['bytes_per_s'] / 1e12:.2f} | {r['hbm_frac']:.2f} |")
