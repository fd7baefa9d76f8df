"""Boundary refinement micro-benchmark (developer tool, GPU): the stage of include/hiseg_refine.h at the C2 mask
size -- 256 x 3 x 128 x 96 logits, bf16 conv chain, eval BatchNorm + ReLU -- and the B0-std train step with and
without the stage.

Per row: us per call from HIP events (WARMUP untimed calls, then the median of REPEATS windows of CALLS calls each).
The stage rows also give the bytes the launches move in HBM by construction (f32 logits in and out, e, the bf16
channel-last copy, the two 32-channel bf16 intermediates written and read, the f32 1x1 output) against the
algorithmic bytes (12 B read + 12 B written per pixel) and the fraction of the 8.0 TB/s HBM peak the call reaches on
the algorithmic bytes.  The windows include launch overhead and the Python wrappers: a call time, not a kernel time.
The stage is timed twice on the same module: the fused kernel (the default for this configuration) and the conv chain
(HISEG_REFINE_FUSED=0).

Prints one JSON object; --markdown adds the table for DESIGN.md.
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

HBM_PEAK = 8.0e12   # bytes / s
WARMUP, REPEATS, CALLS = 5, 7, 10
SHAPE = (256, 3, 128, 96)


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / CALLS)
    return statistics.median(us), min(us), max(us)


def stage_rows():
    """The fused kernel (edge map + one launch) and, with HISEG_REFINE_FUSED=0, the conv chain on the same module."""
    rows = []
    for fused in (True, False):
        os.environ["HISEG_REFINE_FUSED"] = "1" if fused else "0"
        rows.append(stage_row(fused))
    os.environ.pop("HISEG_REFINE_FUSED")
    return rows


def stage_row(fused):
    m = filler.fill_module(hiseg.BoundaryRefinementModule(3, 32, "batchnorm", 8, "relu"))
    m = hiseg.set_compute_dtype(m, torch.bfloat16).cuda().eval()
    x = torch.from_numpy(filler.normal(7, SHAPE) * 2.0).cuda()
    med, lo, hi = timed(lambda: m(x))
    P = SHAPE[0] * SHAPE[2] * SHAPE[3]
    # edge pass: logits in, e out (+ the bf16 channel-last copy for the chain); chain: copy in, two 32-channel bf16
    # intermediates written and read, f32 1x1 output written and read, logits + e in, logits out; fused: logits + e
    # in, logits out (the tile halos re-read 56 % more logits: (20 / 16)^2)
    moved = P * ((12 + 4 + 16 + 16 + 4 * 64 + 16 + 16 + 4 + 12 + 12) if not fused else (12 + 4 + 19 + 4 + 12))
    algo = P * 24
    return {"row": "stage, fused kernel (bf16)" if fused else "stage, conv chain (bf16)", "us": med, "us_min": lo, "us_max": hi, "bytes_moved": moved,
            "bytes_algorithmic": algo, "hbm_frac_algorithmic": algo / (med * 1e-6) / HBM_PEAK}


def step_rows():
    from hiseg import train_engine as TE
    kw = dict(roi_size=(64, 48), mask_size=(128, 96), use_attention_module=True, use_contour_detection=True,
              use_distance_transform=True, normalization_type="batchnorm", activation_function="relu",
              use_pretrained_unet=True, pretrained_weights_path="", freeze_pretrained_weights=True,
              use_full_image_unet=True, encoder_name="timm-efficientnet-b0", hierarchical_base_channels=64,
              hierarchical_depth=3)
    images = torch.from_numpy(filler.uniform(1, (8, 3, 480, 640))).cuda()
    rois = torch.from_numpy(filler.box_rois(2, 8, 4)).cuda()
    tgt = torch.from_numpy(filler.ellipse_targets(3, 32, 128, 96)).cuda()
    rows = []
    for refine in (False, True):
        m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**kw, use_boundary_refinement=refine))
        m = hiseg.set_compute_dtype(m, torch.bfloat16).cuda().train()
        loss_fn = hiseg.RefinedHierarchicalLoss(use_boundary_aware_loss=True, use_contour_detection=True,
                                                use_distance_transform=True, use_active_contour_loss=refine)
        opt = hiseg.FusedAdamW(m, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)

        def step():
            logits, aux = m(images, rois)
            loss, _ = loss_fn(logits, tgt, aux)
            opt.zero_grad()
            loss.backward()
            opt.step()
        med, lo, hi = timed(step)
        rows.append({"row": "B0-std train step, 32 ROIs" + (" + stage + active contour" if refine else ""),
                     "us": med, "us_min": lo, "us_max": hi})
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    rows = stage_rows() + ([] if args.no_step else step_rows())
    print(json.dumps({"shape": SHAPE, "rows": rows}))
    if args.markdown:
        print("| row | us / call (min-max) | bytes moved / algorithmic | HBM frac (algorithmic) |\n|---|---|---|---|")
        for r in rows:
            b = f"{r['bytes_moved'] / 1e6:.0f} / {r['bytes_algorithmic'] / 1e6:.0f} MB" if "bytes_moved" in r else "-"
            f = f"{r['hbm_frac_algorithmic']:.3f}" if "hbm_frac_algorithmic" in r else "-"
            print(f"| {r['row']} | {r['us']:.0f} ({r['us_min']:.0f}-{r['us_max']:.0f}) | {b} | {f} |")
