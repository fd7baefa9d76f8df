"""Golden vectors for the ROI-model knowledge-distillation loss, produced by running the REFERENCE's
DistillationLoss (advanced/knowledge_distillation.py:10-134) on the CPU (build container only; seeded,
single-threaded).

    python tests/golden/gen_kd_golden.py

Writes tests/golden/kd.npz and tests/golden/kd_surface.json (data only).

Inputs are not stored: both sides regenerate them with tests/kd_cases.py ``kd_inputs`` from tests/golden/filler.py (the
extreme case stores its tensors).  Per case ``<shape>_<variant>_T<t>``: ``_keys`` / ``_vals`` the loss dict in the
reference's order (float64), ``_heads`` which of (logits, bg_fg, target_nontarget) entered the distillation term.
The stub base loss has no gradient, so d total / d (student tensor) of a head that ran does not depend on the
variant: it is stored once per (shape, T) from the ``all`` variant as ``<shape>_T<t>_grad<h>`` and every other
variant is asserted here to reproduce it bit for bit (and to give no gradient to a head that did not run).  For
(2,128,96) the gradients are stored at the pixels ``grad_pixels(H * W)`` only (every 8th, and the first and last
128 of each plane), for T = 4.0 and 0.5; the loss values are stored for every temperature.

Variants: ``all`` three heads; ``taux_none`` teacher passed as a bare tensor; ``no_s_bgfg`` / ``no_t_bgfg`` /
``no_s_tn`` / ``no_t_tn`` one aux key missing on one side; ``nologits`` distill_logits=False; ``bare`` the student
passed as a bare tensor with aux_outputs=.  ``all`` is recorded at T = 4.0, 1.0 and 0.5, the others at 4.0.
``<shape>_refined``: the reference's RefinedHierarchicalLoss (fresh EMA state, first call) as the base loss, with
the full gradients.  ``extreme_T<t>``: a teacher pixel (200, -200, 0) whose q underflows to exactly 0, a student
pixel of +-80, and a pixel where student and teacher are equal.
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
sys.path.insert(0, os.path.dirname(HERE))
from kd_cases import (  # noqa: E402  (shared with the tests: shapes, seeded inputs, variants)
    ALPHA, SHAPES, STUB, TEMPS, VARIANTS, call, grad_pixels, kd_inputs, kd_targets, tag, ttag)
from src.human_edge_detection.advanced import knowledge_distillation as KD  # noqa: E402
from src.human_edge_detection.advanced.hierarchical_segmentation_refinement import RefinedHierarchicalLoss  # noqa: E402

torch.set_num_threads(1)
REFINED_SHAPES = ((2, 7, 5), (3, 12, 10))


def extreme_inputs():
    s, t = kd_inputs((1, 2, 4))
    s = [a.copy() for a in s]
    t = [a.copy() for a in t]
    t[0][0, :, 0, 0] = (200.0, -200.0, 0.0)
    t[1][0, :, 0, 0] = (200.0, -200.0)
    t[2][0, :, 0, 0] = (-200.0, 200.0)
    s[0][0, :, 0, 1] = (80.0, -80.0, 0.0)
    s[1][0, :, 0, 1] = (-80.0, 80.0)
    s[2][0, :, 0, 1] = (80.0, -80.0)
    for a, b in zip(s, t):
        a[0, :, 0, 2] = b[0, :, 0, 2]
    s[0][0, :, 1, 0] = (80.0, -80.0, 0.0)   # the +-80 student against the underflowing teacher
    t[0][0, :, 1, 0] = (-200.0, 200.0, 0.0)
    return s, t


class StubBase(torch.nn.Module):
    def forward(self, pred, target, aux=None):
        return torch.tensor(STUB["total_loss"]), dict(STUB)


def run(variant, base, temp, s_np, t_np, target, **kw):
    s = [torch.from_numpy(a.copy()).requires_grad_(True) for a in s_np]
    t = [torch.from_numpy(a.copy()) for a in t_np]
    loss_fn = KD.DistillationLoss(base, temperature=temp, alpha=ALPHA, distill_logits=(variant != "nologits"), **kw)
    total, d, heads = call(variant, loss_fn, s, t, torch.from_numpy(target))
    total.backward()
    assert np.isfinite(float(total)) and all(np.isfinite(float(v)) for v in d.values()), (variant, temp)
    return d, heads, [a.grad for a in s]


def record(out, key, d, heads):
    out[f"{key}_keys"] = np.array(list(d.keys()))
    out[f"{key}_vals"] = np.array([float(v) for v in d.values()], np.float64)
    out[f"{key}_heads"] = np.array(heads, np.uint8)


def gen_stub_cases(out, key_sets):
    for shape in SHAPES:
        s_np, t_np = kd_inputs(shape)
        target = kd_targets(shape)
        hw = shape[1] * shape[2]
        big = shape == SHAPES[-1]
        for temp in TEMPS:
            ref_grads = None
            for variant in VARIANTS if temp == TEMPS[0] else ("all",):
                d, heads, grads = run(variant, StubBase(), temp, s_np, t_np, target)
                key = f"{tag(shape)}_{variant}_{ttag(temp)}"
                record(out, key, d, heads)
                key_sets[variant] = list(d.keys())
                if variant == "all":
                    ref_grads = grads
                    if big and temp == 1.0:
                        continue
                    for h, g in enumerate(grads):
                        g = g.reshape(g.shape[0], g.shape[1], hw)
                        out[f"{tag(shape)}_{ttag(temp)}_grad{h}"] = g[:, :, grad_pixels(hw)] if big else g
                else:
                    for h, g in enumerate(grads):
                        if heads[h]:
                            assert torch.equal(g, ref_grads[h]), (key, h)
                        else:
                            assert g is None, (key, h)


def gen_refined_cases(out, key_sets):
    for shape in REFINED_SHAPES:
        s_np, t_np = kd_inputs(shape)
        d, heads, grads = run("all", RefinedHierarchicalLoss(), 4.0, s_np, t_np, kd_targets(shape))
        key = f"{tag(shape)}_refined"
        record(out, key, d, heads)
        key_sets["refined"] = list(d.keys())
        for h, g in enumerate(grads):
            out[f"{key}_grad{h}"] = g


def gen_extreme(out):
    s_np, t_np = extreme_inputs()
    target = np.zeros((1, 2, 4), np.int64)
    for h in range(3):
        out[f"extreme_s{h}"], out[f"extreme_t{h}"] = s_np[h], t_np[h]
    q = torch.softmax(torch.from_numpy(t_np[0]) / 0.5, dim=1)
    assert float(q[0, 1, 0, 0]) == 0.0 and float(q[0, 2, 0, 0]) == 0.0   # exactly 0
    for temp in (0.5, 4.0):
        d, heads, grads = run("all", StubBase(), temp, s_np, t_np, target)
        key = f"extreme_{ttag(temp)}"
        record(out, key, d, heads)
        for h, g in enumerate(grads):
            assert torch.isfinite(g).all()
            out[f"{key}_grad{h}"] = g


if __name__ == "__main__":
    out = {"alpha": np.array(ALPHA), "temps": np.array(TEMPS), "shapes": np.array(SHAPES),
           "stub_keys": np.array(list(STUB)), "stub_vals": np.array(list(STUB.values()), np.float64),
           "variants": np.array(VARIANTS), "refined_shapes": np.array(REFINED_SHAPES)}
    key_sets = {}
    gen_stub_cases(out, key_sets)
    gen_refined_cases(out, key_sets)
    gen_extreme(out)
    G.save("kd", **out)
    loss = KD.DistillationLoss(StubBase(), feature_match_layers=None)
    wrap = KD.DistillationModelWrapper(torch.nn.Linear(2, 2), torch.nn.Linear(2, 3))
    surface = {
        "ctor_DistillationLoss": list(inspect.signature(KD.DistillationLoss).parameters),
        "ctor_defaults_DistillationLoss": {k: p.default for k, p in
                                           inspect.signature(KD.DistillationLoss).parameters.items()
                                           if p.default is not inspect.Parameter.empty},
        "forward_args_DistillationLoss": list(inspect.signature(KD.DistillationLoss.forward).parameters),
        "ctor_DistillationModelWrapper": list(inspect.signature(KD.DistillationModelWrapper).parameters),
        "ctor_defaults_DistillationModelWrapper": {"freeze_teacher": True},
        "wrapper_methods": sorted(n for n in ("forward", "train", "eval", "get_student", "get_teacher")
                                  if callable(getattr(wrap, n))),
        "wrapper_state_keys": sorted(wrap.state_dict().keys()),
        "feature_match_layers_default": loss.feature_match_layers,
        "dict_keys": key_sets,
    }
    with open(os.path.join(HERE, "kd_surface.json"), "w") as f:
        json.dump(surface, f, indent=0)
