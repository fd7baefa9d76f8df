"""Micro-benchmark of the directional, adaptive and optimized edge-smoothing kernels (developer tool, GPU), modelled on
tools/post_bench.py: 256 x 1 x 128 x 96 instance masks (LDS-resident form) and 32 x 1 x 480 x 640 binary masks (tiled
form, 64x64 tiles with a halo of 2).

Per filter and shape: us per call from HIP events (WARMUP untimed calls, then REPEATS windows of CALLS calls each;
median and min - max of the windows), the bytes moved by construction -- one read and one write of every plane: 8 bytes
per pixel for f32 planes, 4 for the f16 planes of OptimizedEdgeSmoothing(use_fp16=True), 6 when that module is given
f32 masks (the kernel rounds them while it reads; what a serving hook sees) -- and that traffic as a
fraction of the 8.0 TB/s HBM peak (MI355X spec).  The windows include launch overhead and the output allocation of the
Python wrapper: a call time, not a kernel time.  No pass / fail threshold.

Prints one JSON object; --markdown adds the table for DESIGN.md.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "human-instance-segmentation_amd"))
import hiseg  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s
WARMUP, REPEATS, CALLS = 10, 7, 20
SHAPES = {"roi 256x1x128x96 (resident)": (256, 1, 128, 96), "full 32x1x480x640 (tiled)": (32, 1, 480, 640)}


def time_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return statistics.median(windows), min(windows), max(windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(11)
    rows = []
    for sname, shape in SHAPES.items():
        B, _, H, W = shape
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, device=dev), torch.linspace(-1, 1, W, device=dev), indexing="ij")
        field = 1 - ((yy / 0.6) ** 2 + (xx / 0.5) ** 2)
        binary = ((field > 0) ^ (torch.rand(shape, device=dev, generator=gen) < 0.08)).float()
        half = binary.half()
        per_plane = [torch.empty(B, 1, device=dev).uniform_(lo, hi, generator=gen)
                     for lo, hi in ((1.0, 5.0), (0.5, 2.0), (0.3, 0.7))]
        adaptive = hiseg.AdaptiveEdgeSmoothing().to(dev)
        cases = (
            ("edge_smooth (basic, for scale)", hiseg.BinaryMaskEdgeSmoothing().to(dev), binary, 8),
            ("dir_edge_smooth", hiseg.DirectionalEdgeSmoothing().to(dev), binary, 8),
            ("adaptive_edge_smooth (per-plane parameters)", lambda t: adaptive(t, *per_plane), binary, 8),
            ("adaptive_edge_smooth (stride 0)", hiseg.AdaptiveEdgeSmoothing(3.0, 1.0, 0.5).to(dev), binary, 8),
            ("opt_edge_smooth f32", hiseg.OptimizedEdgeSmoothing(use_fp16=False).to(dev), binary, 8),
            ("opt_edge_smooth f16 (f16 planes in)", hiseg.OptimizedEdgeSmoothing(use_fp16=True).to(dev), half, 4),
            ("opt_edge_smooth f16 (f32 masks in: the serving hook)", hiseg.OptimizedEdgeSmoothing(use_fp16=True).to(dev),
             binary, 6),
        )
        for name, fn, x, bpp in cases:
            with torch.no_grad():
                us, lo, hi = time_us(lambda: fn(x))
            moved = B * H * W * bpp
            rows.append({"filter": name, "shape": sname, "us": round(us, 1), "us_min_max": [round(lo, 1), round(hi, 1)],
                         "bytes_moved": moved, "bytes_per_pixel": bpp,
                         "hbm_peak_fraction": round(moved / (us * 1e-6) / HBM_PEAK, 4)})
    print(json.dumps({"hbm_peak_Bps": HBM_PEAK, "warmup": WARMUP, "repeats": REPEATS, "calls": CALLS, "rows": rows}))
    if args.markdown:
        print("| filter | shape | us per call (min - max) | MB moved | HBM peak fraction |")
        print("|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['filter']} | {r['shape']} | {r['us']} ({r['us_min_max'][0]} - {r['us_min_max'][1]}) | "
                  f"{r['bytes_moved'] / 1e6:.1f} | {100 * r['hbm_peak_fraction']:.1f} % |")


if __name__ == "__main__":
    main()
