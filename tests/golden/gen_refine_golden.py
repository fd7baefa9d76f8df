"""Golden vectors for the boundary refinement stage and the active-contour loss, produced by running the REFERENCE
on the CPU (build container only; seeded, single-threaded, reproducible bit for bit).

    python tests/golden/gen_refine_golden.py

Writes tests/golden/refine.npz and tests/golden/state_keys_refine.json (data only: weights come from
tests/golden/filler.py, blend_weight is set to BLEND in every fixture -- with the default 0.01 the stage moves the
logits by ~3e-3 and a test could not tell it from a no-op).

* module cases -- BoundaryRefinementModule (advanced/hierarchical_segmentation_refinement.py:58-149): input,
  normalised edge map E, output in eval mode (batchnorm and layernorm2d; batchnorm + SiLU for `odd` and `big`) and, in train mode (batchnorm), the output
  and the gradients of the input, blend_weight and every edge_conv parameter for a seeded upstream gradient.
  `min` (2,3,2,3) is the smallest legal size, `odd` (3,3,9,7) an odd one, `big` (2,3,40,36) spans several
  workgroups, `const` takes the E = 0 branch, `flat` carries a 4x4 patch of identical logit triples: the
  reference's input gradient is NaN there (sqrt backward at 0) and the mask of it is stored.
* active contour -- min(active_contour_loss(softmax(pred)), 10) (:347-386, :920-925) and its gradient at
  (2,3,2,2) (both curvature terms 0), (2,3,3,5) and (2,3,32,24).  The clamp at 10 cannot be reached: the term is
  built from differences of probabilities, so it is at most 2 + 0.01 * 4 = 2.04; no such fixture exists.
* head and step -- the B0-std model of gen_train_golden.py (UNet logits injected, dropout off) with
  use_boundary_refinement=True: eval forward, then one train step under RefinedHierarchicalLoss with the active
  contour and boundary-aware terms on.
* per eval case the error of the reference under CPU bf16 autocast against its own f32 run (the bf16 tests' bar).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (installs the smp stand-in, imports the reference)
import filler  # noqa: E402

torch.set_num_threads(1)
R = G.R
BLEND = 0.3
MODULE_CASES = {   # name: (seed, shape)
    "min": (102, (2, 3, 2, 3)), "odd": (111, (3, 3, 9, 7)), "big": (121, (2, 3, 40, 36)),
    "const": (131, (2, 3, 9, 7)), "flat": (141, (2, 3, 12, 10)),
}
AC_CASES = {"ac_small": (201, (2, 3, 2, 2)), "ac_odd": (211, (2, 3, 3, 5)), "ac_mask": (221, (2, 3, 32, 24))}
LOSS_KW = dict(bg_weight=1.5, fg_weight=1.5, target_weight=1.2, consistency_weight=0.3, use_dynamic_weights=True,
               dice_weight=1.0, ce_weight=1.0, active_contour_weight=0.1, boundary_aware_weight=0.1,
               contour_loss_weight=0.1, distance_loss_weight=0.1, use_active_contour_loss=True,
               use_boundary_aware_loss=True, use_contour_detection=True, use_distance_transform=True)
DICT_KEYS = ["bg_fg_loss", "target_nontarget_loss", "final_loss", "consistency_loss", "total_loss", "ce_loss",
             "dice_loss", "aux_fg_bg_loss", "aux_fg_accuracy", "aux_fg_iou", "bg_weight", "fg_weight",
             "target_weight", "nontarget_weight", "active_contour", "boundary_aware", "contour", "contour_weight",
             "distance_transform"]


def case_input(name):
    seed, shape = MODULE_CASES[name]
    if name == "const":
        x = np.broadcast_to(np.array([0.7, -1.1, 0.2], np.float32)[None, :, None, None], shape).copy()
    else:
        x = filler.normal(seed, shape) * 2.0
    if name == "flat":
        x[1, :, 3:7, 2:6] = np.array([0.5, -0.25, 1.5], np.float32)[:, None, None]
    return torch.from_numpy(x), torch.from_numpy(filler.normal(seed + 1, shape))


def make_module(norm, act="relu"):
    m = filler.fill_module(R.BoundaryRefinementModule(3, 32, norm, 8, act, 1.0))
    with torch.no_grad():
        m.blend_weight.fill_(BLEND)
    return m


def raw_edges(x):
    p = torch.softmax(x, 1)
    dy = torch.nn.functional.pad((p[:, :, 1:] - p[:, :, :-1]).abs(), (0, 0, 0, 1), mode="replicate")
    dx = torch.nn.functional.pad((p[:, :, :, 1:] - p[:, :, :, :-1]).abs(), (0, 1, 0, 0), mode="replicate")
    return torch.sqrt(dy ** 2 + dx ** 2).mean(1)


def gen_modules(out):
    for name in MODULE_CASES:
        x, g = case_input(name)
        out[f"{name}_x"], out[f"{name}_g"] = x, g
        if name not in ("const",):
            e = raw_edges(x)
            n_img = e[0].numel()
            assert int(e.argmin()) // n_img != int(e.argmax()) // n_img, f"{name}: change the seed (same sample)"
            if name != "flat":   # (the flat patch ties the min at 0 on purpose: there the tie rule decides)
                assert int((e == e.min()).sum()) == 1 and int((e == e.max()).sum()) == 1, f"{name}: change the seed (tie)"
        for norm in ("batchnorm", "layernorm2d"):
            m = make_module(norm).eval()
            with torch.no_grad():
                y = m(x)
                E = m.detect_edges(x)
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    yb = m(x).float()
            tag = "bn" if norm == "batchnorm" else "ln"
            out[f"{name}_{tag}_eval_out"] = y
            out[f"{name}_{tag}_eval_bf16_err"] = ((yb - x) - (y - x)).abs().max()
            if norm == "batchnorm":
                out[f"{name}_E"] = E
        if name == "const":
            assert torch.equal(y, x) and float(E.abs().max()) == 0.0
        if name in ("odd", "big"):   # a module outside the fused kernel's case: batchnorm + SiLU
            m = make_module("batchnorm", "silu").eval()
            with torch.no_grad():
                y = m(x)
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    yb = m(x).float()
            out[f"{name}_bnsilu_eval_out"] = y
            out[f"{name}_bnsilu_eval_bf16_err"] = ((yb - x) - (y - x)).abs().max()
        m = make_module("batchnorm").train()
        xr = x.clone().requires_grad_(True)
        y = m(xr)
        (y * g).sum().backward()
        out[f"{name}_bn_train_out"] = y.detach()
        dx = xr.grad
        if name == "flat":
            nan = torch.isnan(dx)
            assert nan.any() and not nan.all()
            out["flat_dx_nan"] = nan
            dx = torch.where(nan, torch.zeros_like(dx), dx)
        else:
            assert torch.isfinite(dx).all()
        if name == "const":
            assert torch.equal(dx, g)
        out[f"{name}_dx"] = dx
        names = [n for n, _ in m.named_parameters()]
        out[f"{name}_grad_names"] = np.array(names)
        for n, p in m.named_parameters():
            assert torch.isfinite(p.grad).all(), (name, n)
            out[f"{name}_grad_{n}"] = p.grad
        for n, b in m.named_buffers():
            if "running_" in n:
                out[f"{name}_buf_{n}"] = b


def gen_active_contour(out):
    for name, (seed, shape) in AC_CASES.items():
        pred = torch.from_numpy(filler.normal(seed, shape) * 2.0).requires_grad_(True)
        loss = torch.clamp(R.active_contour_loss(torch.softmax(pred, 1), smoothness_weight=0.01), max=10.0)
        loss.backward()
        out[f"{name}_pred"], out[f"{name}_loss"], out[f"{name}_grad"] = pred.detach(), loss.detach(), pred.grad


def sample(t, k=64):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // k)
    return f[::step][:k].clone()


def gen_step(out, kw):
    kw = dict(kw, use_boundary_refinement=True)
    torch.manual_seed(0)
    model = G.build_ref_model(kw)
    with torch.no_grad():
        model.segmentation_head.boundary_refiner.blend_weight.fill_(BLEND)
    with open(os.path.join(HERE, "state_keys_refine.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in model.segmentation_head.state_dict().items()
                   if k.startswith("boundary_refiner.")}, f, indent=0)
    for m in model.modules():
        if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)):
            m.p = 0.0
    images = torch.from_numpy(filler.uniform(61, (2, 3, 96, 128)))
    u = torch.from_numpy(filler.normal(62, (2, 1, 96, 128)) * 2.0)
    rois = torch.tensor([[0, .10, .10, .40, .90], [1, .35, .15, .80, .95], [0, .55, .05, .95, .70]], dtype=torch.float32)
    for m in (model.roi_align_mask, model.roi_align_rgb):
        m.spatial_scale, m.spatial_scale_h, m.spatial_scale_w = (96, 128), 96, 128
    mh, mw = G.tup(kw["mask_size"])
    tgt = torch.from_numpy(filler.ellipse_targets(63, 3, mh, mw))
    G._InjectedUnet.injected = u
    with torch.no_grad():
        logits, aux = model(images, rois)
        head = model.segmentation_head
        head.use_boundary_refinement = False
        base, _ = model(images, rois)
        head.use_boundary_refinement = True
    differ = int(((logits.argmax(1) == 1) != (base.argmax(1) == 1)).sum())
    assert differ >= 1, "the refiner changes no instance-mask pixel: change the fixture"
    out["step_eval_logits"], out["step_eval_base_logits"] = sample(logits, 4096), sample(base, 4096)
    out["step_eval_bgfg"] = sample(aux["bg_fg_logits"], 4096)
    out["step_eval_mask_pixels_changed"] = np.array(differ)
    out["step_eval_instance_sum"] = (logits.argmax(1) == 1).sum(dim=(1, 2))
    model.train()
    loss_fn = R.RefinedHierarchicalLoss(**LOSS_KW)
    logits, aux = model(images, rois)
    loss, d = loss_fn(logits, tgt, aux)
    loss.backward()
    out["step_logits"] = sample(logits, 4096)
    out["step_bgfg"] = sample(aux["bg_fg_logits"], 4096)
    out["step_tn"] = sample(aux["target_nontarget_logits"], 4096)
    out["step_contours"] = sample(aux["contours"], 4096)
    out["step_loss"] = loss.detach()
    out["step_dict"] = np.array([float(d.get(k, np.nan)) for k in DICT_KEYS])
    out["step_dict_keys"] = np.array(DICT_KEYS)
    params = dict(model.named_parameters())
    names = [n for n in params if ".boundary_refiner." in n]
    names += ["segmentation_head.base_head.shared_features.0.weight", "pretrained_unet.output_conv.weight",
              "pretrained_unet.output_conv.bias"]
    out["step_grad_names"] = np.array(names)
    for n in names:   # the refiner's gradients whole, the large shared conv's as sum of squares + strided sample
        g = params[n].grad
        if g.numel() > 16384:
            out[f"step_gradsq_{n}"] = np.array(float((g.double() ** 2).sum()))
            g = sample(g, 1024)
        out[f"step_grad_{n}"] = g
    br = model.segmentation_head.boundary_refiner
    for n, b in br.named_buffers():
        if "running_" in n or n.endswith("num_batches_tracked"):
            out[f"step_buf_{n}"] = b


if __name__ == "__main__":
    cfgs = json.load(open(os.path.join(HERE, "configs.json")))
    out = {"blend": np.array(BLEND, np.float32)}
    gen_modules(out)
    gen_active_contour(out)
    gen_step(out, cfgs["b0"]["model_kwargs"])
    G.save("refine", **out)
