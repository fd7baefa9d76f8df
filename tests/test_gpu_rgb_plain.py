"""Plain RGB model and the hierarchical head at any mask size on the GPU, against the reference's golden vectors
(tests/golden/rgb_plain.npz, tests/golden/gen_rgb_plain_golden.py).

f32: logits and every aux tensor within the project's f32 bar (1e-4 of the tensor's magnitude, as
tests/test_gpu_parity.py), the instance masks equal to the reference's argmax outside the pixels whose top two
reference logits are closer than that bar (at most 0.1 % of a case's pixels, asserted), roi_patches within the
RoIAlign bar of tests/test_gpu_parity.py (1e-5).  bf16: the error against the f32 fixture is at most twice the
reference's own CPU-bf16-autocast error of that case and tensor, plus the f32 bar (tests/test_gpu_refine.py's rule).
Large tensors are compared on the fixture's strided sample.
"""
import numpy as np
import pytest
import torch

import filler
from helpers import b0_kwargs, hiseg_kwargs, load

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_TOL = 1e-4
HEAD_CASES = {   # name: (N, roi size, mask size) -- tests/golden/gen_rgb_plain_golden.py
    "x2": (2, (4, 4), (8, 8)), "half": (2, (4, 8), (4, 8)), "ratio": (2, (8, 12), (11, 20)),
    "up": (2, (8, 8), (20, 20)), "odd": (3, (12, 8), (17, 13)),
}
REFINED_CASES = {"rsame": (2, (8, 12), (8, 12)), "rratio": (2, (8, 12), (11, 20))}
MODEL_MASKS = {"m2x": (16, 24), "msame": (8, 12), "mratio": (11, 20)}
NORMS = {"ln": "layernorm2d", "bn": "batchnorm"}
HEAD_KEYS = [f"{n}_{a}" for n in HEAD_CASES for a in ("att", "noatt")] + \
            [f"{n}_{t}" for n in REFINED_CASES for t in ("bn", "ln")]
MODEL_KEYS = [f"{n}_{t}" for n in MODEL_MASKS for t in ("ln", "bn")]


@pytest.fixture(scope="module")
def G():
    return load("rgb_plain")


def _sample(t, k=4096):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // k)
    return f[::step][:k]


def _figures(G, key, logits, aux, bf16):
    """{tensor: (error on the fixture's sample, bar)} for the logits and every aux tensor of the fixture."""
    keys = [str(k) for k in G[f"{key}_aux_keys"]]
    assert set(aux) == set(keys), (sorted(aux), keys)
    figs = {}
    for k, v in dict(aux, logits=logits).items():
        assert tuple(v.shape) == tuple(G[f"{key}_{k}_shape"]), k
        e = (_sample(v).double().cpu() - torch.from_numpy(G[f"{key}_{k}"]).double()).abs().max().item()
        bar = F32_TOL * max(1.0, float(G[f"{key}_{k}_absmax"]))
        if bf16:
            bar = 2.0 * float(G[f"{key}_{k}_bf16_err"]) + bar
        elif k == "roi_patches":
            bar = 1e-5
        figs[k] = (e, bar)
    return figs


def _check(G, key, logits, aux, dt):
    bf16 = dt == torch.bfloat16
    figs = _figures(G, key, logits, aux, bf16)
    print(f"rgb plain {key} {dt}: " + ", ".join(f"{k} {e:.2e}/{b:.2e}" for k, (e, b) in figs.items()))
    for k, (e, b) in figs.items():
        assert e <= b if bf16 else e < b, (k, e, b)
    if not bf16:
        _check_masks(G, key, logits)


def _unpack(bits, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(bits)[:n].astype(bool).reshape(shape))


def _check_masks(G, key, logits):
    """argmax == 1 equals the reference's outside the pixels whose top two reference logits are within the f32 bar."""
    from hiseg import ops
    shape = (logits.shape[0],) + tuple(logits.shape[2:])
    close, ref = _unpack(G[f"{key}_close"], shape), _unpack(G[f"{key}_inst"], shape)
    assert close.float().mean().item() <= 1e-3
    inst = ops.instance_masks(logits).cpu()[:, 0] > 0.5
    assert torch.equal(inst[~close], ref[~close]), key


def _head(key, dt):
    import hiseg
    name, tag = key.split("_")
    ms_of = lambda ms: ms[0] if ms[0] == ms[1] else ms   # noqa: E731
    if name in HEAD_CASES:
        N, (h, w), ms = HEAD_CASES[name]
        head = hiseg.HierarchicalSegmentationHeadUNetV2(256, 256, 3, ms_of(ms), use_attention_module=tag == "att")
    else:
        N, (h, w), ms = REFINED_CASES[name]
        head = hiseg.RefinedHierarchicalSegmentationHead(
            256, 256, 3, ms_of(ms), use_attention_module=True, use_boundary_refinement=True,
            use_contour_detection=True, use_distance_transform=True, normalization_type=NORMS[tag])
    return hiseg.set_compute_dtype(filler.fill_module(head).eval().to(DEV), dt), (N, 256, h, w)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("key", HEAD_KEYS)
def test_head_matches_reference(G, key, dt):
    head, shape = _head(key, dt)
    x = torch.from_numpy(filler.normal(int(G[f"{key}_seed"]), shape)).to(DEV)
    logits, aux = head(x)
    torch.cuda.synchronize()
    assert ("shared_features" in aux) == (key.split("_")[0] in REFINED_CASES)
    _check(G, key, logits, aux, dt)


def _model(key, dt):
    import hiseg
    name, tag = key.split("_")
    m = hiseg.create_rgb_hierarchical_model(roi_size=(8, 12), mask_size=MODEL_MASKS[name],
                                            normalization_type=NORMS[tag], use_attention_module=True)
    m = filler.fill_module(m).eval().to(DEV)
    m.roi_align.spatial_scale_h, m.roi_align.spatial_scale_w = 64, 96
    return hiseg.set_compute_dtype(m, dt)


def _model_inputs(G, key):
    return (torch.from_numpy(filler.uniform(int(G[f"{key}_seed"]), (2, 3, 64, 96))).to(DEV),
            torch.from_numpy(G["model_rois"]).to(DEV))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("key", MODEL_KEYS)
def test_model_matches_reference(G, key, dt):
    images, rois = _model_inputs(G, key)
    model = _model(key, dt)
    logits, aux = model(images, rois)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (3, 3) + MODEL_MASKS[key.split("_")[0]]
    _check(G, key, logits, aux, dt)
    assert torch.equal(model.infer(images, rois), logits)   # infer: the same kernels, no aux tensors


def _count_combines(monkeypatch):
    from hiseg import ops
    calls = {"hier_combine": 0, "hier_combine_resize": 0}
    for name in calls:
        def wrapper(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrapper)
    return calls


def _full_image_model(mask, dt=torch.float32):
    import hiseg
    kw = hiseg_kwargs(b0_kwargs())
    kw.update(roi_size=(8, 12), mask_size=mask)
    m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**kw)).eval().to(DEV)
    for r in (m.roi_align_mask, m.roi_align_rgb):
        r.spatial_scale_h, r.spatial_scale_w = 64, 96
    return hiseg.set_compute_dtype(m, dt)


def test_full_image_model_runs_at_mask_equal_to_roi(G, monkeypatch):
    images, rois = _model_inputs(G, "msame_ln")
    calls = _count_combines(monkeypatch)
    logits, aux = _full_image_model((8, 12))(images, rois)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (3, 3, 8, 12) and torch.isfinite(logits).all()
    assert calls == {"hier_combine": 0, "hier_combine_resize": 1}
    for k in ("bg_fg_logits", "target_nontarget_logits", "contours", "distance_map", "distance_mask"):
        assert tuple(aux[k].shape[2:]) == (8, 12), k


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_twice_the_roi_still_takes_hier_combine(G, monkeypatch, dt):
    """mask = 2 x ROI launches hiseg_hier_combine, as before, and not the new kernel -- in the full-image model and
    in the plain one."""
    images, rois = _model_inputs(G, "m2x_ln")
    calls = _count_combines(monkeypatch)
    logits, _ = _full_image_model((16, 24), dt)(images, rois)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (3, 3, 16, 24)
    assert calls == {"hier_combine": 1, "hier_combine_resize": 0}
    _model("m2x_bn", dt).infer(images, rois)
    assert calls == {"hier_combine": 2, "hier_combine_resize": 0}
    _model("mratio_bn", dt).infer(images, rois)
    assert calls == {"hier_combine": 2, "hier_combine_resize": 1}


@pytest.mark.parametrize("key", ["mratio_bn", "msame_ln"])
def test_infer_replays_bit_identically_from_a_graph(G, key):
    images, rois = _model_inputs(G, key)
    model = _model(key, torch.bfloat16)
    eager = model.infer(images, rois)   # builds the plans
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.infer(images, rois)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits = model.infer(images, rois)
    for _ in range(2):
        logits.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(logits, eager)


def test_composer_accepts_the_plain_models_logits(G):
    import hiseg
    images, rois = _model_inputs(G, "mratio_ln")
    logits = _model("mratio_ln", torch.bfloat16).infer(images, rois)
    imap, score = hiseg.InstanceMapComposer(frame_size=(2, 64, 96))(logits, rois)
    torch.cuda.synchronize()
    assert tuple(imap.shape) == (2, 64, 96) and imap.dtype == torch.int32
    assert tuple(score.shape) == (rois.shape[0],) and 0 <= int(imap.min()) and int(imap.max()) <= rois.shape[0]
