"""UNet-guided direct 3-class head on the GPU against the reference's golden vectors (tests/golden/unet_guided_head.npz).

f32: logits and every aux tensor within the project's f32 bar (1e-4 of the tensor's magnitude, as
tests/test_gpu_parity.py), the instance masks equal to the reference's argmax outside the pixels whose top two
reference logits are closer than that bar (at most 0.1 % of a case's pixels).  bf16: the error against the f32 fixture
is at most twice the reference's own CPU-bf16-autocast error of that case and tensor, plus the f32 bar (the existing
bf16 bars' rule, tests/test_gpu_refine.py: the tensors the reference computes from the f32 mask logits under autocast
have a stored error of 0, and a bf16 run is not asked to beat the f32 bar on them).  The fused forms are bit-identical
to their explicit fall-backs, the serving paths to the serial module, a captured graph to its eager run.
"""
import numpy as np
import pytest
import torch

import filler
from helpers import b0_kwargs, hiseg_kwargs, load

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_TOL = 1e-4
HEAD_CASES = {   # name: (seed, N, roi size, mask size) -- tests/golden/gen_unet_guided_head_golden.py
    "min": (302, 2, (2, 3), (4, 6)), "odd": (311, 3, (9, 7), (18, 14)), "same": (321, 2, (8, 12), (8, 12)),
    "big": (331, 2, (20, 18), (40, 36)), "ratio": (341, 2, (6, 8), (9, 20)),
}
VARIANTS = {"bn": ("batchnorm", "relu"), "ln": ("layernorm2d", "relu"), "bnsilu": ("batchnorm", "silu")}
AUX_KEYS = ("bg_fg_logits", "target_nontarget_logits", "fg_prob", "pretrained_bg_fg_mask", "attention")
HEAD_PARAMS = [(n, t, a) for n in HEAD_CASES for t in (("bn", "ln", "bnsilu") if n == "odd" else ("bn",))
               for a in (True, False)]
FLAGS = ("use_boundary_refinement", "use_progressive_upsampling", "use_subpixel_conv", "use_contour_detection",
         "use_distance_transform")


@pytest.fixture(scope="module")
def G():
    return load("unet_guided_head")


def _err(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(np.asarray(ref)).double()
    return (a - ref).abs().max().item()


def _bar(ref, absmax=None):
    m = float(np.abs(np.asarray(ref)).max()) if absmax is None else float(absmax)
    return F32_TOL * max(1.0, m)


def _head(name, tag, att, dt):
    import hiseg
    norm, act = VARIANTS[tag]
    ms = HEAD_CASES[name][3]
    h = hiseg.PretrainedUNetGuidedSegmentationHead(256, 256, 3, ms[0] if ms[0] == ms[1] else ms,
                                                   use_attention_module=att, normalization_type=norm,
                                                   normalization_groups=8, activation_function=act)
    return hiseg.set_compute_dtype(filler.fill_module(h).eval().to(DEV), dt)


def _head_inputs(G, name):
    seed, N, (h, w), _ = HEAD_CASES[name]
    return (torch.from_numpy(filler.normal(seed, (N, 256, h, w))).to(DEV),
            torch.from_numpy(G[f"{name}_mask"]).to(DEV))


def _unpack(bits, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(bits)[:n].astype(bool).reshape(shape))


def _check_masks(G, key, logits):
    """argmax == 1 equals the reference's outside the pixels whose top two reference logits are within the f32 bar."""
    shape = (logits.shape[0],) + tuple(logits.shape[2:])
    close, ref = _unpack(G[f"{key}_close"], shape), _unpack(G[f"{key}_inst"], shape)
    assert close.float().mean().item() <= 1e-3
    from hiseg import ops
    inst = ops.instance_masks(logits).cpu()[:, 0] > 0.5
    assert torch.equal(inst[~close], ref[~close]), key


@pytest.mark.parametrize("name,tag,att", HEAD_PARAMS)
def test_head_matches_reference_f32(G, name, tag, att):
    key = f"{name}_{tag}_{'att' if att else 'noatt'}"
    x, mask = _head_inputs(G, name)
    logits, aux = _head(name, tag, att, torch.float32)(x, mask)
    torch.cuda.synchronize()
    assert set(aux) == set(AUX_KEYS)
    figures = {"logits": (_err(logits, G[f"{key}_logits"]), _bar(G[f"{key}_logits"]))}
    for k in AUX_KEYS:
        if k == "attention" and not att:
            assert aux[k] is None
            continue
        assert tuple(aux[k].shape) == G[f"{key}_{k}"].shape, k
        figures[k] = (_err(aux[k], G[f"{key}_{k}"]), _bar(G[f"{key}_{k}"]))
    print(f"guided head f32 {key}: " + ", ".join(f"{k} {e:.2e}/{b:.2e}" for k, (e, b) in figures.items()))
    for k, (e, b) in figures.items():
        assert e < b, (k, e, b)
    _check_masks(G, key, logits)
    assert torch.equal(aux["target_nontarget_logits"], logits[:, 1:3])
    if name == "same":   # nothing resized: the raw mask logit and the ROI-size fg_prob
        assert torch.equal(aux["pretrained_bg_fg_mask"], mask[:, 1:2])


@pytest.mark.parametrize("name,tag,att", HEAD_PARAMS)
def test_head_bf16_within_twice_the_reference_autocast_error(G, name, tag, att):
    key = f"{name}_{tag}_{'att' if att else 'noatt'}"
    x, mask = _head_inputs(G, name)
    logits, aux = _head(name, tag, att, torch.bfloat16)(x, mask)
    torch.cuda.synchronize()
    outs = dict(aux, logits=logits)
    ratios = {}
    for k in ("logits",) + AUX_KEYS:
        if outs[k] is None:
            continue
        ref, stored = G[f"{key}_{k}"], float(G[f"{key}_{k}_bf16_err"])
        e = _err(outs[k], ref)
        ratios[k] = (e, stored, 2.0 * stored + _bar(ref))
    print(f"guided head bf16 {key}: " + ", ".join(
        f"{k} {e:.2e} (ref autocast {s:.2e}, ratio {e / s if s else float('nan'):.2f})" for k, (e, s, _) in ratios.items()))
    for k, (e, _, bar) in ratios.items():
        assert e <= bar, (k, e, bar)


def _model(dt, **over):
    import hiseg
    kw = hiseg_kwargs(b0_kwargs())
    kw.update({f: False for f in FLAGS})
    kw.update(over)
    m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**kw)).eval().to(DEV)
    for r in (m.roi_align_mask, m.roi_align_rgb):
        r.spatial_scale_h, r.spatial_scale_w = 96, 128
    return hiseg.set_compute_dtype(m, dt)


def _model_inputs(G):
    return (torch.from_numpy(filler.uniform(351, (2, 3, 96, 128))).to(DEV),
            torch.from_numpy(filler.normal(352, (2, 1, 96, 128)) * 2.0).to(DEV),
            torch.from_numpy(G["model_rois"]).to(DEV))


def _sample(t, k=4096):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // k)
    return f[::step][:k]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_model_matches_reference(G, dt):
    from hiseg import engine
    images, u, rois = _model_inputs(G)
    model = _model(dt)
    logits, aux = engine.rgb_model_forward(model, images, rois, "full", unet_logit_override=u)
    torch.cuda.synchronize()
    keys = [str(k) for k in G["model_aux_keys"]]
    assert set(keys) <= set(aux) and set(aux) - set(keys) <= {"attention"}
    outs = dict(aux, logits=logits)
    figs = {}
    for k in ["logits"] + keys:
        ref = G[f"model_{k}"]
        e = _err(_sample(outs[k]), ref)
        bar = _bar(ref, G[f"model_{k}_absmax"])
        stored = float(G[f"model_{k}_bf16_err"])
        figs[k] = (e, bar if dt == torch.float32 else 2.0 * stored + bar, stored)
    print(f"guided model {dt}: " + ", ".join(f"{k} {e:.2e}/{b:.2e} (autocast {s:.2e})" for k, (e, b, s) in figs.items()))
    for k, (e, b, _) in figs.items():
        assert e <= b if dt == torch.bfloat16 else e < b, (k, e, b)
    if dt == torch.float32:
        _check_masks(G, "model", logits)
        # model.infer and model(...) are the same kernels
        l2, a2 = model(images, rois)
        assert set(a2) == set(aux)
        l3, _ = model.infer(images, rois)
        assert torch.equal(l2, l3)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("norm", ["batchnorm", "layernorm2d"])
def test_fused_forms_are_bit_identical_to_their_fallbacks(G, dt, norm):
    """px_scale attention (the gate multiply in final_classifier.0's loader) against an explicit scale pass, and
    fg_prob as loader source B against a materialised 257-channel input (asked for in f32; bf16 rides along)."""
    from hiseg import engine
    images, u, rois = _model_inputs(G)
    model = _model(dt, normalization_type=norm)
    outs = {}
    try:
        for px, sb in ((True, True), (False, True), (True, False)):
            engine.GUIDED_FUSE_PX_SCALE, engine.GUIDED_FUSE_SRC_B = px, sb
            logits, aux = engine.rgb_model_forward(model, images, rois, "full", unet_logit_override=u)
            torch.cuda.synchronize()
            outs[(px, sb)] = (logits, aux)
    finally:
        engine.GUIDED_FUSE_PX_SCALE = engine.GUIDED_FUSE_SRC_B = True
    ref_l, ref_a = outs[(True, True)]
    assert torch.isfinite(ref_l).all()
    for k, (l, a) in outs.items():
        assert torch.equal(l, ref_l), k
        for n in AUX_KEYS:
            assert torch.equal(a[n], ref_a[n]), (k, n)


def test_fg_prob_is_loader_source_b_of_input_adjust(G):
    """The 257-channel input never exists: input_adjust reads the features as source A and the one-channel fg_prob
    (one 16-byte chunk per pixel) as source B.  final_classifier.0 is a 3x3 layer, for which the library has no
    per-pixel loader scale (hiseg_conv2d_fused_ok: the pointwise kernel alone), so ops.conv2d(px_scale=) runs its
    explicit pixel_scale pass there -- no launch carries px_scale."""
    from hiseg import engine, ops
    images, u, rois = _model_inputs(G)
    model = _model(torch.bfloat16)
    engine.rgb_model_forward(model, images, rois, "none", unet_logit_override=u)
    ops.RECORD = []
    try:
        engine.rgb_model_forward(model, images, rois, "none", unet_logit_override=u)
        rec = ops.RECORD
    finally:
        ops.RECORD = None
    assert sum(1 for d, *_ in rec if d.srcB and d.KH == 1 and d.Cb == 8) == 1
    assert sum(1 for d, *_ in rec if d.KH == 1 and d.Ca + d.Cb > 256 and not d.srcB) == 0
    assert not any(d.px_scale for d, *_ in rec)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_aux_none_logits_are_bit_identical_and_write_no_aux(G, dt):
    from hiseg import engine
    images, u, rois = _model_inputs(G)
    model = _model(dt)
    full, aux = engine.rgb_model_forward(model, images, rois, "full", unet_logit_override=u)
    none, aux_none = engine.rgb_model_forward(model, images, rois, "none", unet_logit_override=u)
    torch.cuda.synchronize()
    assert torch.equal(full, none)
    assert set(aux_none) == {"unet_logit"}


def test_export_wrapper_and_stream_pipeline_equal_the_serial_module():
    import hiseg
    from hiseg import ops
    model = _model(torch.bfloat16)
    batches = [(torch.from_numpy(filler.uniform(400 + k, (2, 3, 96, 128))).to(DEV),
                torch.from_numpy(filler.box_rois(500 + k, 2, 2)).to(DEV)) for k in range(3)]
    comp = hiseg.InstanceMapComposer()
    wrap = hiseg.RGBHierarchicalExportWrapper(model, dilation_pixels=1, binary_post=hiseg.BinaryMaskEdgeSmoothing(),
                                              instance_post=hiseg.BinaryMaskEdgeSmoothing(), compose=comp)
    plain = hiseg.RGBHierarchicalExportWrapper(model, dilation_pixels=1)
    with torch.no_grad():
        serial = [wrap(i, r) for i, r in batches]
        piped = hiseg.StreamPipelinedExport(wrap).run(batches)
        for (images, rois), out in zip(batches, serial):
            logits, unet = model.infer(images, rois)          # the serial module outputs
            inst = ops.instance_masks(logits, 1)
            pi, pb = plain(images, rois)
            assert torch.equal(pi, inst)
            oc = model.pretrained_unet.output_conv
            assert torch.equal(pb, ops.binary_masks(unet, oc.weight.detach().view(2).contiguous(),
                                                    oc.bias.detach().contiguous()))
            assert torch.equal(out[0], wrap.instance_post(inst)) and torch.equal(out[1], wrap.binary_post(pb))
            assert out[2].shape == (2, 96, 128) and out[2].dtype == torch.int32
    torch.cuda.synchronize()
    for a, b in zip(serial, piped):
        assert len(a) == len(b) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_forward_replays_bit_identically_from_a_graph(G):
    from hiseg import engine
    images, u, rois = _model_inputs(G)
    model = _model(torch.bfloat16)
    eager, _ = engine.rgb_model_forward(model, images, rois, "full", unet_logit_override=u)   # builds the plans
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        engine.rgb_model_forward(model, images, rois, "full", unet_logit_override=u)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits, aux = engine.rgb_model_forward(model, images, rois, "full", unet_logit_override=u)
    for _ in range(2):
        logits.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(logits, eager)
    assert torch.isfinite(aux["bg_fg_logits"]).all()
