"""Golden vectors for the distance-aware segmentation loss, produced by running the REFERENCE on the CPU (build
container only; seeded, single-threaded, scipy 1.15.3).

    python tests/golden/gen_distance_golden.py

Writes tests/golden/distance.npz and tests/golden/distance_surface.json (data only).

* weight-map cases -- DistanceTransform.compute_boundary_distance and BoundaryWeightGenerator.generate_weights
  (advanced/distance_aware_loss.py:13-50, :147-185) per mask, for the widths 1, 3, 5, 8 and the weight pairs
  (2.0, 3.0) and (1.2, 2.5): `<case>_t` the masks (uint8), `<case>_d2_w<width>` the squared clipped distance
  (uint8: the reference's float64 distance squared and rounded, asserted to be an integer), `<case>_w_w<width>_p<pair>`
  the f32 weights.  Masks: 1x1, 1x7, 7x1, 2x3, 9x7; 40x36 with all three classes; 56x56 with {0,1}; 64x48 with
  {1,2}; all-0, all-1, all-2 and {0,2} (no site at all, or every pixel a site); `pyth`, one site with pixels at
  d2 = 20, 25 (3-4-5 and 5-0) and 26 -- 24 is not a sum of two squares, so no pixel of a grid can lie at it, and
  20 = 4^2 + 2^2 is the nearest value below 25 that exists; `mixed`, a batch of a three-class and a two-class
  sample (the site rule is per sample).  `<case>_dist64` for 9x7 and 40x36: the transform with max_distance 64.
* loss cases -- DistanceAwareSegmentationLoss / AdaptiveBoundaryLoss (:188-373) at (3,3,12,10) (`s_`) and
  (2,3,40,36) (`b_`): targets, logits, instance maps, then per variant the weight map, d2, the loss-dict values
  (`_vals`, in the order of `dict_keys`; the adaptive variants append boundary_weight and instance_weight) and
  d total / d pred.
* the factory's class weights for PIXEL_RATIOS.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (puts the reference on sys.path)
import filler  # noqa: E402
from src.human_edge_detection.advanced import distance_aware_loss as D  # noqa: E402

torch.set_num_threads(1)
WIDTHS = (1, 3, 5, 8)
PAIRS = ((2.0, 3.0), (1.2, 2.5))
PIXEL_RATIOS = {"background": 0.485, "target": 0.393, "non_target": 0.122}
DICT_KEYS = ["total_loss", "ce_loss", "dice_loss", "boundary_accuracy", "avg_boundary_weight"]


def rand_mask(seed, h, w, classes=(0, 1, 2)):
    rng = np.random.default_rng(seed)
    m = rng.choice(np.array(classes), size=(h, w))
    flat = m.reshape(-1)
    if flat.size >= len(classes):
        flat[:len(classes)] = classes   # every class present
    return m.astype(np.int64)


def masks():
    e40 = filler.ellipse_targets(301, 1, 40, 36)[0]
    assert set(np.unique(e40)) == {0, 1, 2}
    e56 = filler.ellipse_targets(302, 1, 56, 56)[0]
    e56[e56 == 2] = 0
    e64 = filler.ellipse_targets(303, 1, 64, 48)[0]
    e64[e64 == 0] = 2
    assert set(np.unique(e56)) == {0, 1} and set(np.unique(e64)) == {1, 2}
    m02 = np.zeros((8, 8), np.int64)
    m02[2:5, 3:] = 2
    pyth = np.zeros((12, 12), np.int64)
    pyth[0, 0] = 1
    mixed = np.stack([rand_mask(311, 12, 10), rand_mask(312, 12, 10, (0, 1))])
    return {"m1x1": np.ones((1, 1, 1), np.int64), "m1x7": rand_mask(304, 1, 7)[None], "m7x1": rand_mask(305, 7, 1)[None],
            "m2x3": rand_mask(306, 2, 3)[None], "m9x7": rand_mask(307, 9, 7)[None], "m40x36": e40[None],
            "m56x56": e56[None], "m64x48": e64[None], "all0": np.zeros((1, 8, 8), np.int64),
            "all1": np.ones((1, 8, 8), np.int64), "all2": np.full((1, 8, 8), 2, np.int64), "m02": m02[None],
            "pyth": pyth[None], "mixed": mixed}


def ref_d2(mask, width):
    d = D.DistanceTransform.compute_boundary_distance(torch.from_numpy(mask), max_distance=width).numpy()
    d2 = np.rint(d * d)
    assert np.abs(d * d - d2).max() < 1e-9 and d2.max() <= width * width
    return d2.astype(np.uint8)


def gen_weight_maps(out):
    for name, ms in masks().items():
        out[f"{name}_t"] = ms.astype(np.uint8)
        for width in WIDTHS:
            out[f"{name}_d2_w{width}"] = np.stack([ref_d2(m, width) for m in ms])
            for pi, (bw, isw) in enumerate(PAIRS):
                gen = D.BoundaryWeightGenerator(width, bw, isw)
                w = torch.stack([gen.generate_weights(torch.from_numpy(m), None) for m in ms])
                assert w.dtype == torch.float32
                out[f"{name}_w_w{width}_p{pi}"] = w
    d2 = out["pyth_d2_w8"][0]
    assert (d2[4, 2], d2[3, 4], d2[5, 0], d2[5, 1]) == (20, 25, 25, 26)
    w5 = out["pyth_w_w5_p0"][0]
    assert w5[4, 2] > 1 and w5[3, 4] == 1 and w5[5, 0] == 1 and w5[5, 1] == 1   # d2 == width^2 falls outside
    z = out["all0_w_w5_p0"][0]   # the virtual site at (-1, 0) of a mask without sites
    assert np.allclose(z[0, :3], [1.8, 1.7171573, 1.5527864]) and np.allclose(z[1, :2], [1.6, 1.5527864])
    for name in ("m9x7", "m40x36"):
        m = torch.from_numpy(masks()[name][0])
        out[f"{name}_dist64"] = D.DistanceTransform.compute_boundary_distance(m, max_distance=64.0)


def loss_inputs(tag):
    if tag == "s":
        t = filler.ellipse_targets(321, 3, 12, 10)
        t[1][t[1] == 2] = 0
        x = filler.normal(322, (3, 3, 12, 10)) * 2.0
        assert set(np.unique(t[0])) == {0, 1, 2} and set(np.unique(t[1])) == {0, 1}
    else:
        t = filler.ellipse_targets(331, 2, 40, 36)
        x = filler.normal(332, (2, 3, 40, 36)) * 2.0
    n, h, w = t.shape
    straddle = filler.uniform(323 if tag == "s" else 333, (n, h, w), 30.0, 70.0)
    straddle[:, 0, 0] = 50.0   # exactly 50 is not "close"
    straddle[:, 0, 1] = np.nextafter(np.float32(50.0), np.float32(0.0))
    return t, x, straddle


def variants(tag, straddle):
    n = straddle.shape[0]
    cw = D.create_distance_aware_loss(PIXEL_RATIOS).class_weights
    zeros = [{"instance_distances": torch.zeros(straddle.shape[1:])} for _ in range(n)]
    strad = [{"instance_distances": torch.from_numpy(straddle[i])} for i in range(n)]
    missing = [dict(d) for d in strad]
    missing[1] = {}
    v = {"plain": (dict(), None), "cw": (dict(class_weights=cw), None),
         "focal2": (dict(class_weights=cw, use_focal=True, focal_gamma=2.0), None),
         "focal15": (dict(use_focal=True, focal_gamma=1.5, ce_weight=0.7, dice_weight=1.3), None),
         "adaptive": (dict(class_weights=cw, adaptive=(6.5, 0.5)), strad)}
    if tag == "s":
        v.update({"inst_zeros": (dict(), zeros), "inst_straddle": (dict(boundary_width=3), strad),
                  "inst_missing": (dict(class_weights=cw), missing),
                  "adaptive_plain": (dict(adaptive=(2.25, 3.0), boundary_width=8), None),
                  "nob": (dict(boundary_width=1, boundary_weight=1.2), None),
                  "tied": (dict(boundary_width=5, boundary_weight=3.0), None)})
    return v


def gen_losses(out):
    for tag in ("s", "b"):
        t, x, straddle = loss_inputs(tag)
        out[f"{tag}_t"], out[f"{tag}_x"], out[f"{tag}_straddle"] = t.astype(np.uint8), x, straddle
        for name, (kw, info) in variants(tag, straddle).items():
            kw = dict(kw)
            adaptive = kw.pop("adaptive", None)
            xs = x.copy()
            if name == "tied":   # two-way ties (classes 0 and 1, 1 and 2) and a three-way tie, on boundary pixels
                xs[:, 1, 3:6, :] = xs[:, 0, 3:6, :]
                xs[:, 0, 3:6, :] = np.maximum(xs[:, 0, 3:6, :], xs[:, 2, 3:6, :] + 0.5)
                xs[:, 1, 3:6, :] = xs[:, 0, 3:6, :]
                xs[:, 2, 6:8, :] = xs[:, 1, 6:8, :] = np.maximum(xs[:, 1, 6:8, :], xs[:, 0, 6:8, :] + 0.5)
                xs[:, :, 8, :] = 0.25
                out[f"{tag}_{name}_x"] = xs
            loss_fn = D.DistanceAwareSegmentationLoss(**kw)
            if adaptive is not None:
                loss_fn = D.AdaptiveBoundaryLoss(loss_fn)
                with torch.no_grad():
                    loss_fn.boundary_weight.fill_(adaptive[0])
                    loss_fn.instance_weight.fill_(adaptive[1])
            pred = torch.from_numpy(xs).requires_grad_(True)
            total, d = loss_fn(pred, torch.from_numpy(t), info)
            total.backward()
            keys = DICT_KEYS + (["boundary_weight", "instance_weight"] if adaptive is not None else [])
            assert set(d.keys()) == set(keys)
            out[f"{tag}_{name}_vals"] = np.array([float(d[k]) for k in keys], np.float64)
            out[f"{tag}_{name}_grad"] = pred.grad
            gen = (loss_fn.base_loss if adaptive is not None else loss_fn).weight_generator
            w = torch.stack([gen.generate_weights(torch.from_numpy(t[i]), info[i] if info else None)
                             for i in range(len(t))])
            out[f"{tag}_{name}_w"] = w
            out[f"{tag}_{name}_d2"] = np.stack([ref_d2(m, gen.boundary_width) for m in t])
            if name == "nob":
                assert float(w.max()) <= 1.5 and float(d["boundary_accuracy"]) == 0.0
            if name == "tied":
                b = w > 1.5
                am = pred.detach().argmax(1)
                tie = (xs.max(1, keepdims=True) == xs).sum(1) > 1
                assert (torch.from_numpy(tie) & b).sum() > 8, "the ties must lie on boundary pixels"
                assert ((am == 0) & torch.from_numpy(tie) & b).any() and ((am == 1) & torch.from_numpy(tie) & b).any()


if __name__ == "__main__":
    out = {"dict_keys": np.array(DICT_KEYS), "widths": np.array(WIDTHS), "pairs": np.array(PAIRS),
           "pixel_ratios": np.array([PIXEL_RATIOS[k] for k in ("background", "target", "non_target")])}
    out["factory_class_weights"] = D.create_distance_aware_loss(PIXEL_RATIOS).class_weights
    gen_weight_maps(out)
    gen_losses(out)
    G.save("distance", **out)
    ad = D.create_distance_aware_loss(PIXEL_RATIOS, adaptive=True)
    surface = {
        "adaptive_state_keys": sorted(ad.state_dict().keys()),
        "ctor_DistanceAwareSegmentationLoss": list(inspect.signature(D.DistanceAwareSegmentationLoss).parameters),
        "ctor_AdaptiveBoundaryLoss": list(inspect.signature(D.AdaptiveBoundaryLoss).parameters),
        "factory_args": list(inspect.signature(D.create_distance_aware_loss).parameters),
        "forward_args": list(inspect.signature(D.DistanceAwareSegmentationLoss.forward).parameters),
    }
    with open(os.path.join(HERE, "distance_surface.json"), "w") as f:
        json.dump(surface, f, indent=0)
