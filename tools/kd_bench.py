#!/usr/bin/env python3
"""Timing of the ROI-model knowledge distillation (hiseg.DistillationLoss / DistillationModelWrapper) on one GPU.

    python tools/kd_bench.py [--rois 256] [--rounds 5] [--iters 200] [--steps 10] [--no-step]

Prints one JSON line.

* ``term``: the KD term alone at N ROIs of 128x96 (the C2 / B0 batch): the fused forward (two launches) and
  backward (one launch) through the C ABI with their achieved GB/s (14 floats read per pixel forward, 14 read and 7
  written backward), the fused forward + backward through hiseg.DistillationLoss's autograd node, and the same
  term composed from torch ops (log_softmax / softmax / kl_div and autograd), which is what a user would write
  without the kernels.  The variants are timed interleaved, ``rounds`` times ``iters`` calls each between device
  events; the median over the rounds and the min-max spread are reported.
* ``step``: the B0-std train step (32 images 640x480, 8 ROIs each, bf16, FusedAdamW, eager launches) without
  distillation, and with a frozen B3-encoder teacher and the KD loss with ``overlap_teacher`` False and True,
  interleaved the same way.

No GPU: fails (a CPU run measures nothing about the MI355X).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "human-instance-segmentation_amd"), os.path.join(ROOT, "tests", "golden"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

MASK_HW = (128, 96)
AUX = ("bg_fg_logits", "target_nontarget_logits")


def timed_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def interleaved(variants, rounds, iters, warmup):
    """{name: (median ms, min ms, max ms)} of callables timed round-robin."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed_ms(fn, iters))
    return {k: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in t.items()}


def term_bench(n, rounds, iters):
    import torch.nn.functional as F

    import hiseg
    from hiseg import _lib as L
    lib = L.lib()
    dev = torch.device("cuda")
    h, w = MASK_HW
    g = torch.Generator(device=dev).manual_seed(0)
    s = [(torch.randn(n, c, h, w, device=dev, generator=g) * 2).requires_grad_(True) for c in (3, 2, 2)]
    t = [torch.randn(n, c, h, w, device=dev, generator=g) * 2 for c in (3, 2, 2)]
    T, alpha = 4.0, 0.7
    ws = torch.empty(int(lib.hiseg_kd_ws(n, h, w)), device=dev)
    out = torch.empty(4, device=dev)
    d = [torch.empty_like(a) for a in s]
    gs = torch.tensor([alpha], device=dev)
    td = torch.tensor([T], device=dev)
    ptrs = [x[i].data_ptr() for i in range(3) for x in (s, t)]
    stream = L.stream_ptr()

    def raw_fwd():
        L.check(lib.hiseg_kd_loss_fwd(*ptrs, n, h, w, 0.0, td.data_ptr(), ws.data_ptr(), out.data_ptr(), stream),
                "kd_loss_fwd")

    def raw_bwd():
        L.check(lib.hiseg_kd_loss_bwd(*ptrs, n, h, w, 0.0, td.data_ptr(), gs.data_ptr(), d[0].data_ptr(),
                                      d[1].data_ptr(), d[2].data_ptr(), stream), "kd_loss_bwd")
    base = torch.zeros((), device=dev)
    loss_fn = hiseg.DistillationLoss(lambda pred, target, aux=None: (base, {}), temperature=T, alpha=alpha)

    def fused():
        total, _ = loss_fn((s[0], dict(zip(AUX, s[1:]))), (t[0], dict(zip(AUX, t[1:]))), None)
        torch.autograd.grad(total, s)

    def composed():
        kd = 0
        for i, wgt in enumerate((1.0, 0.3, 0.3)):
            kd = kd + F.kl_div(F.log_softmax(s[i] / T, dim=1), F.softmax(t[i] / T, dim=1),
                               reduction="batchmean") * (T ** 2) * wgt
        total = alpha * kd + (1 - alpha) * base
        torch.autograd.grad(total, s)
    r = interleaved({"fused_fwd": raw_fwd, "fused_bwd": raw_bwd, "fused_module_fwd_bwd": fused,
                     "torch_composed_fwd_bwd": composed}, rounds, iters, warmup=20)
    px = n * h * w
    r["fused_fwd"]["gb_per_s"] = 14 * 4 * px / (r["fused_fwd"]["ms"] * 1e-3) / 1e9
    r["fused_bwd"]["gb_per_s"] = 21 * 4 * px / (r["fused_bwd"]["ms"] * 1e-3) / 1e9
    r["bytes_fwd"], r["bytes_bwd"] = 14 * 4 * px, 21 * 4 * px
    return r


def step_bench(rounds, steps, batch=32, per_image=8, hw=(480, 640), teacher_encoder="timm-efficientnet-b3"):
    import filler
    import hiseg
    from bench import B0_KWARGS
    dev = torch.device("cuda")

    def build(kw, seed):
        m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**kw), seed=seed).to(dev)
        for mm in (m.roi_align_mask, m.roi_align_rgb):
            mm.spatial_scale_h, mm.spatial_scale_w = hw
        return hiseg.set_compute_dtype(m, torch.bfloat16)
    student = build(B0_KWARGS, 0)
    tkw = dict(B0_KWARGS, encoder_name=teacher_encoder, freeze_pretrained_weights=False)
    wrap = hiseg.DistillationModelWrapper(build(tkw, 5), student).train()
    images = torch.rand(batch, 3, *hw, generator=torch.Generator().manual_seed(0)).to(dev)
    rois = torch.from_numpy(filler.box_rois(1, batch, per_image)).to(dev)
    tgt = torch.from_numpy(filler.ellipse_targets(7, batch * per_image, *MASK_HW)).to(dev)

    def refined():
        return hiseg.RefinedHierarchicalLoss(use_boundary_aware_loss=True, use_contour_detection=True,
                                             use_distance_transform=True, boundary_aware_weight=0.1,
                                             contour_loss_weight=0.1, distance_loss_weight=0.1)
    base_fn, kd_fn = refined(), hiseg.DistillationLoss(refined(), temperature=4.0, alpha=0.7)
    state = {"opt": None}

    def finish(loss):
        if state["opt"] is None:
            state["opt"] = hiseg.FusedAdamW(student, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0)
        state["opt"].zero_grad()
        loss.backward()
        state["opt"].step()

    def plain():
        logits, aux = student(images, rois)
        finish(base_fn(logits, tgt, aux)[0])

    def kd(overlap):
        def run():
            wrap.overlap_teacher = overlap
            s_out, t_out = wrap(images, rois)
            finish(kd_fn(s_out, t_out, tgt)[0])
        return run
    r = interleaved({"plain": plain, "kd_serial": kd(False), "kd_overlap": kd(True)}, rounds, steps, warmup=3)
    r["rois"] = batch * per_image
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kd_bench: no GPU")
    out = {"device": torch.cuda.get_device_name(0), "term": term_bench(args.rois, args.rounds, args.iters)}
    if not args.no_step:
        out["step"] = step_bench(args.rounds, args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
