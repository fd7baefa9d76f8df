"""Distance-aware loss micro-benchmark (developer tool, GPU): forward plus backward of
hiseg.DistanceAwareSegmentationLoss at the ROI count and mask size of bench.py's B0 train preset (256 ROI samples,
128 x 96 masks) against the reference's method restated -- torch ops on the GPU for the cross entropy, the Dice term
and autograd, and for the weight map the per-ROI host loop of advanced/distance_aware_loss.py:13-50, :147-185
(mask.cpu().numpy(), np.unique, scipy's distance_transform_edt, a copy back).  The baseline is skipped, saying so,
when scipy cannot be imported.

ms per call from HIP events for hiseg (WARMUP untimed calls, then the median of REPEATS windows of CALLS calls) and
from the wall clock around a synchronised call for the baseline (its time is host work).  The two are compared once
(weight map bit for bit, loss to 1e-5) so that both columns time the same function.  Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "human-instance-segmentation_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
import hiseg  # noqa: E402
import filler  # noqa: E402

WARMUP, REPEATS, CALLS = 5, 7, 10
N, H, W = 256, 128, 96


def baseline_weights(targets, width, bw, edt):
    out = torch.ones_like(targets, dtype=torch.float32)
    for i in range(targets.shape[0]):   # the reference's loop: one host round trip per ROI
        m = targets[i].cpu().numpy()
        if len(np.unique(m)) > 2:
            dy = np.abs(np.diff(m, axis=0, prepend=m[0:1]))
            dx = np.abs(np.diff(m, axis=1, prepend=m[:, 0:1]))
            edges = ((dy > 0) | (dx > 0)).astype(np.float32)
        else:
            edges = m.astype(np.float32)
        dist = torch.from_numpy(np.minimum(edt(1 - edges), width)).to(targets.device)
        near = dist < width
        w = torch.ones_like(dist, dtype=torch.float32)
        w[near] *= (1.0 + (bw - 1.0) * (1.0 - dist / width))[near]
        out[i] = w
    return out


def baseline_step(pred, targets, width, bw, edt):
    pred = pred.detach().requires_grad_(True)
    ce = F.cross_entropy(pred, targets, reduction="none")
    w = baseline_weights(targets, width, bw, edt)
    wce = (ce * w).mean()
    p1 = torch.softmax(pred, 1)[:, 1]
    t1 = (targets == 1).float()
    dice = (1 - (2 * (p1 * t1).sum((1, 2)) + 1e-6) / (p1.sum((1, 2)) + t1.sum((1, 2)) + 1e-6)).mean()
    total = wce + dice
    total.backward()
    return total.detach(), w, pred.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=N)
    args = ap.parse_args()
    dev = torch.device("cuda")
    n = args.rois
    targets = torch.from_numpy(filler.ellipse_targets(5, n, H, W)).to(dev)
    pred = (torch.from_numpy(filler.normal(6, (n, 3, H, W))) * 2).to(dev)
    loss_fn = hiseg.DistanceAwareSegmentationLoss()

    def step():
        x = pred.detach().requires_grad_(True)
        total, _ = loss_fn(x, targets)
        total.backward()
        return total.detach(), x.grad

    for _ in range(WARMUP):
        step()
    windows = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            step()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / CALLS)
    res = {"workload": f"{n} x 3 x {H} x {W} logits, boundary_width 5, forward + backward",
           "hiseg_ms": round(statistics.median(windows), 4), "hiseg_ms_windows": [round(v, 4) for v in windows]}
    try:
        from scipy.ndimage import distance_transform_edt as edt
    except ImportError:
        res["baseline"] = "skipped: scipy is not importable here"
    else:
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bt, bw_map, bg = baseline_step(pred, targets, 5, 2.0, edt)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        total, grad = step()
        res["baseline_ms"] = round(statistics.median(times), 2)
        res["weight_map_equal"] = bool(torch.equal(bw_map, loss_fn.last["weights"]))
        res["loss_rel_diff"] = float((total - bt).abs() / bt.abs())
        res["grad_rel_diff"] = float((grad - bg).abs().max() / bg.abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
