"""Golden vectors for the UNet-guided direct 3-class head, produced by running the REFERENCE on the CPU (build
container only; seeded, single-threaded, reproducible bit for bit).

    python tests/golden/gen_unet_guided_head_golden.py

Writes tests/golden/unet_guided_head.npz and tests/golden/state_keys_unet_guided_head.json (data only: weights come
from tests/golden/filler.py, which also fills the BatchNorm running statistics with non-trivial values).

* head cases -- PretrainedUNetGuidedSegmentationHead (advanced/hierarchical_segmentation_rgb.py:43-218), eval mode,
  256 channels, batchnorm + relu, each with and without the attention module:
    `min`   (2, 2x3 -> 4x6)     every pixel is a border pixel of the 3x3 convs and of the bilinear clamp
    `odd`   (3, 9x7 -> 18x14)   odd size; also with layernorm2d and with batchnorm + silu
    `same`  (2, 8x12 -> 8x12)   no resize anywhere, fg_prob is not recomputed
    `big`   (2, 20x18 -> 40x36) spans several workgroups
    `ratio` (2, 6x8 -> 9x20)    general bilinear resize
  Features come from filler.normal(seed); the 2-channel mask logits are stored.  They reach |x| ~ 20, so that
  log(1 - p + 1e-7) reaches its floor log(1e-7) (asserted).  Between a logit of about 10 and 17
  the reference's own p = sigmoid(x) sits a few ulp below 1 and log(1 - p + 1e-7) moves by up to 0.1 when the
  logit moves by one ulp; a resized logit is only reproducible to a few ulp, so the mask seed is advanced until no
  pixel of the case changes by more than a quarter of the f32 bar under a +-4 ulp perturbation of the resized logit.
* per case and tensor the error of the reference under CPU bf16 autocast against its own f32 run (`*_bf16_err`).
* per case the pixels whose top two reference logits are closer than the f32 bar (`*_close`, bit-packed) -- at most
  0.1 % of the case's pixels (asserted) -- and the reference's instance mask argmax == 1 (`*_inst`, bit-packed).
* model case -- the B0 kwargs of configs.json with every refinement flag off (UNet logits injected, 2 images of
  96x128, 3 ROIs, RoIAlign scales (96, 128)): eval forward, logits and aux sampled as gen_refine_golden.py does.
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
from src.human_edge_detection.advanced import hierarchical_segmentation_rgb as RGB  # noqa: E402

torch.set_num_threads(1)
F32_BAR = 1e-4
HEAD_CASES = {   # name: (seed, N, roi size, mask size)
    "min": (302, 2, (2, 3), (4, 6)), "odd": (311, 3, (9, 7), (18, 14)), "same": (321, 2, (8, 12), (8, 12)),
    "big": (331, 2, (20, 18), (40, 36)), "ratio": (341, 2, (6, 8), (9, 20)),
}
VARIANTS = {"bn": ("batchnorm", "relu"), "ln": ("layernorm2d", "relu"), "bnsilu": ("batchnorm", "silu")}
AUX_KEYS = ("bg_fg_logits", "target_nontarget_logits", "fg_prob", "pretrained_bg_fg_mask", "attention")


def case_tags(name):
    tags = ["bn"] + (["ln", "bnsilu"] if name == "odd" else [])
    return [(t, att) for t in tags for att in (True, False)]


def make_head(tag, att, mask_size):
    norm, act = VARIANTS[tag]
    ms = mask_size[0] if mask_size[0] == mask_size[1] else mask_size
    return filler.fill_module(RGB.PretrainedUNetGuidedSegmentationHead(
        256, 256, 3, ms, use_attention_module=att, normalization_type=norm, normalization_groups=8,
        activation_function=act, activation_beta=1.0)).eval()


def bar(ref):
    return F32_BAR * max(1.0, float(ref.abs().max()))


def bgfg_of(m):
    p = torch.sigmoid(m)
    return torch.cat([torch.log((1 - p) + 1e-7), torch.log(p + 1e-7)], 1)


def mask_is_stable(mask, mask_size, delta=0.0):
    """No pixel's bg_fg_logits moves by more than a quarter of the f32 bar when the (resized) logit moves by up to
    4 ulp (see the module docstring), or by ``delta`` where the logit itself is only reproducible to that."""
    m = mask[:, 1:2]
    if tuple(m.shape[2:]) != tuple(mask_size):
        m = torch.nn.functional.interpolate(m, size=mask_size, mode="bilinear", align_corners=False)
    ref = bgfg_of(m)
    lim = 0.25 * bar(ref)
    if delta and max(float((bgfg_of(m + delta) - ref).abs().max()), float((bgfg_of(m - delta) - ref).abs().max())) > lim:
        return False
    up, dn = m.clone(), m.clone()
    for _ in range(4):
        up = torch.nextafter(up, torch.full_like(up, float("inf")))
        dn = torch.nextafter(dn, torch.full_like(dn, float("-inf")))
        if float((bgfg_of(up) - ref).abs().max()) > lim or float((bgfg_of(dn) - ref).abs().max()) > lim:
            return False
    return True


def case_mask(name):
    seed, N, (h, w), ms = HEAD_CASES[name]
    for k in range(200):
        m = filler.normal(seed + 1 + 1000 * k, (N, 2, h, w)) * 7.0
        # planted saturated pixels: log(1 - p + 1e-7) reaches its floor whatever the draw
        m[0, 1, 0, 0], m[0, 1, h - 1, w - 1] = 21.0, -21.0
        m[N - 1, 1, 0, :2], m[N - 1, 1, h - 1, w - 2:] = 20.0, -20.0
        m = torch.from_numpy(m)
        if mask_is_stable(m, ms):
            return m
    raise AssertionError(f"{name}: no stable mask in 200 seeds")


def pack(b):
    return np.packbits(b.numpy().astype(np.uint8).reshape(-1))


def close_and_inst(logits):
    top = logits.topk(2, dim=1).values
    close = (top[:, 0] - top[:, 1]) < bar(logits)
    frac = float(close.float().mean())
    assert frac <= 1e-3, f"{frac:.2e} of the pixels have their top two logits within the f32 bar: change the seed"
    return pack(close), pack(logits.argmax(1) == 1)


def gen_heads(out):
    floor = float(torch.log(torch.tensor(1e-7)))
    for name, (seed, N, (h, w), ms) in HEAD_CASES.items():
        x = torch.from_numpy(filler.normal(seed, (N, 256, h, w)))
        mask = case_mask(name)
        out[f"{name}_mask"] = mask
        for tag, att in case_tags(name):
            head = make_head(tag, att, ms)
            with torch.no_grad():
                logits, aux = head(x, mask)
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    lb, ab = head(x, mask)
            key = f"{name}_{tag}_{'att' if att else 'noatt'}"
            out[f"{key}_logits"] = logits
            out[f"{key}_logits_bf16_err"] = (lb.float() - logits).abs().max()
            out[f"{key}_close"], out[f"{key}_inst"] = close_and_inst(logits)
            for k in AUX_KEYS:
                if aux[k] is None:
                    assert k == "attention" and not att
                    continue
                out[f"{key}_{k}"] = aux[k]
                out[f"{key}_{k}_bf16_err"] = (ab[k].float() - aux[k]).abs().max()
            b = aux["bg_fg_logits"]
            assert float(b[:, 0].min()) == floor, f"{name}: log(1 - p + 1e-7) does not reach its floor"
            assert torch.equal(aux["target_nontarget_logits"], logits[:, 1:3])
            if (h, w) == tuple(ms):
                assert torch.equal(aux["fg_prob"], torch.sigmoid(mask[:, 1:2]))
                assert torch.equal(aux["pretrained_bg_fg_mask"], mask[:, 1:2])


def sample(t, k=4096):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // k)
    return f[::step][:k].clone()


def gen_model(out, kw):
    kw = dict(kw)
    for f in ("use_boundary_refinement", "use_progressive_upsampling", "use_subpixel_conv", "use_contour_detection",
              "use_distance_transform"):
        kw[f] = False
    torch.manual_seed(0)
    model = G.build_ref_model(kw)
    assert isinstance(model.segmentation_head, RGB.PretrainedUNetGuidedSegmentationHead)
    assert not hasattr(model, "feature_combiner")
    head = model.segmentation_head
    with open(os.path.join(HERE, "state_keys_unet_guided_head.json"), "w") as f:
        json.dump({"head": {k: list(v.shape) for k, v in head.state_dict().items()},
                   "head_noatt": {k: list(v.shape) for k, v in make_head("bn", False, (4, 6)).state_dict().items()},
                   "model": {k: list(v.shape) for k, v in model.state_dict().items()},
                   "final_bias_init": [float(v) for v in RGB.PretrainedUNetGuidedSegmentationHead(
                       256, 256, 3, 56).final_classifier[3].bias]}, f, indent=0)
    images = torch.from_numpy(filler.uniform(351, (2, 3, 96, 128)))
    u = torch.from_numpy(filler.normal(352, (2, 1, 96, 128)) * 2.0)
    rois = torch.tensor([[0, .10, .10, .40, .90], [1, .35, .15, .80, .95], [0, .55, .05, .95, .70]], dtype=torch.float32)
    for m in (model.roi_align_mask, model.roi_align_rgb):
        m.spatial_scale, m.spatial_scale_h, m.spatial_scale_w = (96, 128), 96, 128
    G._InjectedUnet.injected = u
    with torch.no_grad():
        logits, aux = model(images, rois)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            lb, ab = model(images, rois)
    # the RoIAligned logit is reproducible to ~1e-5 (tests/test_gpu_parity.py), not to a few ulp
    assert mask_is_stable(aux["roi_features"], model.mask_size, delta=2e-5), "model: change the u seed"
    out["model_rois"] = rois   # images / u are regenerated from the filler seeds 351 / 352 by the tests
    out["model_logits"] = sample(logits)
    out["model_logits_absmax"] = logits.abs().max()
    out["model_logits_bf16_err"] = (lb.float() - logits).abs().max()
    out["model_close"], out["model_inst"] = close_and_inst(logits)
    out["model_inst_bf16_agree"] = ((lb.float().argmax(1) == 1) == (logits.argmax(1) == 1)).float().mean()
    for k, v in aux.items():
        if v is None:
            continue
        out[f"model_{k}"] = sample(v)
        out[f"model_{k}_absmax"] = v.abs().max()
        out[f"model_{k}_bf16_err"] = (ab[k].float() - v).abs().max()
    out["model_aux_keys"] = np.array([k for k, v in aux.items() if v is not None])


if __name__ == "__main__":
    cfgs = json.load(open(os.path.join(HERE, "configs.json")))
    out = {}
    gen_heads(out)
    gen_model(out, cfgs["b0"]["model_kwargs"])
    G.save("unet_guided_head", **out)
