"""The guided filter on the GPU (hiseg.EdgePreservingFilter over hiseg_guided_filter_fwd) against the reference's
EdgePreservingFilter evaluated in float64 (tests/golden/guided.npz, written by gen_guided_golden.py), and the
post-filter hooks of the serving wrapper and of StreamPipelinedExport.

Bar per recorded case: max |GPU - gold| <= max(2 * ref32_err, 2e-6), ref32_err being the distance of the
reference's own f32 forward from its float64 forward on that case (stored beside the gold): the kernel may be at
most twice as far from the exact answer as the accepted f32 behaviour, with a floor of about 16 f32 ulps at 1.0
for the cases where the reference is nearly exact.

Shapes: tiny 2x1x2x3 (every window larger than the plane), odd 3x1x37x53 and roi 2x1x48x64 (resident form: at most
6826 pixels), big 1x1x200x264 (tiled form, several tiles in both axes).  The bitwise comparison of the two forms
adds 20x300 and 130x50 planes: still resident, but 5 tile columns / 3 to 5 tile rows in the tiled form.
"""
import os

import numpy as np
import pytest
import torch

import filler
from conftest import GOLDEN
from gen_guided_golden import SETTINGS, guided_inputs
from helpers import b0_kwargs, hiseg_kwargs

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2e-6

_cache = {}


def _gold():
    if "npz" not in _cache:
        _cache["npz"] = dict(np.load(os.path.join(GOLDEN, "guided.npz")))
    return _cache["npz"]


def _case_inputs(shape, mode, kind):
    g = _gold()
    x, guide = guided_inputs(g[f"in/soft_{shape}"], g.get(f"in/rgb_{shape}"), mode, kind)
    return torch.from_numpy(x).to(DEV), None if guide is None else torch.from_numpy(guide).to(DEV)


@pytest.mark.parametrize("shape", ("tiny", "odd", "roi", "big"))
def test_recorded_cases_are_within_twice_the_reference_f32_error(shape):
    import hiseg
    g = _gold()
    names = [str(n) for n in g["cases"] if str(n).endswith("/" + shape)]
    assert len(names) == {"tiny": 24, "odd": 8, "roi": 7, "big": 1}[shape]
    failed = []
    for name in names:
        mode, kind, tag, _ = name.split("/")
        radius, eps = SETTINGS[tag]
        x, guide = _case_inputs(shape, mode, kind)
        got = hiseg.EdgePreservingFilter(radius, eps).to(DEV)(x, guide)
        gold = g[f"gold/{name}"]
        assert tuple(got.shape) == gold.shape and got.dtype == torch.float32, name
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - gold).max())
        ref32 = g[f"err32/{name}"].item()
        bar = max(2 * ref32, FLOOR)
        print(f"guided {name}: max |GPU - gold| {err:.3e}, ref32_err {ref32:.3e}, bar {bar:.3e}")
        if not err <= bar:
            failed.append((name, err, bar))
    assert not failed, failed


def _all_modes(shape):
    for mode in ("self", "m1g3", "x3g1", "x3g3"):
        for kind in ("soft", "bin"):
            yield mode, kind, _case_inputs(shape, mode, kind)


@pytest.mark.parametrize("shape", ("tiny", "odd", "roi"))
def test_tiled_form_gives_the_bits_of_the_resident_form(shape):
    """Out-of-image a / b on the halo and any dependence on the tile position show here."""
    from hiseg import ops
    for mode, kind, (x, guide) in _all_modes(shape):
        for tag, (radius, eps) in SETTINGS.items():
            a = ops.guided_filter(x, guide, radius, eps)
            b = ops.guided_filter(x, guide, radius, eps, force_tiled=True)
            assert torch.equal(a, b), (shape, mode, kind, tag, (a - b).abs().max().item())


@pytest.mark.parametrize("hw", ((20, 300), (130, 50)))
def test_tiled_form_with_several_tiles_gives_the_bits_of_the_resident_form(hw):
    from hiseg import ops
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(2, 1, *hw, generator=gen).to(DEV)
    guide = torch.rand(2, 3, *hw, generator=gen).to(DEV)
    for radius, eps in (*SETTINGS.values(), (1, 0.1), (7, 1e-3), (12, 1e-2), (16, 1e-2)):
        for gd in (None, guide):
            a = ops.guided_filter(x, gd, radius, eps)
            b = ops.guided_filter(x, gd, radius, eps, force_tiled=True)
            assert torch.isfinite(a).all() and torch.equal(a, b), (hw, radius, gd is None, (a - b).abs().max().item())


def test_input_forms_agree():
    import hiseg
    from hiseg import ops
    mod = hiseg.EdgePreservingFilter(4, 1e-3).to(DEV)
    x, guide = _case_inputs("odd", "m1g3", "soft")
    keep_x, keep_g = x.clone(), guide.clone()
    y = mod(x)
    assert torch.equal(mod(x, x), y) and torch.equal(mod(x, x.clone()), y)         # guide = x is self-guided
    assert torch.equal(ops.guided_filter(x, x, 4, 1e-3, force_tiled=True), y)
    y3 = mod(x[0])                                                                 # (C, H, W)
    assert y3.shape == (1, 37, 53) and torch.equal(y3, y[0])
    yg = mod(x, guide)
    yg3 = mod(x[1], guide[1])
    assert yg.shape == (3, 3, 37, 53) and yg3.shape == (3, 37, 53) and torch.equal(yg3, yg[1])
    # a plane that is broadcast gives what its materialised copies give
    assert torch.equal(mod(x.expand(-1, 3, -1, -1), guide), yg)
    assert torch.equal(mod(guide, x.expand(-1, 3, -1, -1).contiguous()), mod(guide, x))
    # non-contiguous inputs give what their contiguous copies give; the inputs are untouched
    wide = torch.zeros(3, 3, 37, 106, device=DEV)
    wide[..., ::2] = guide
    assert torch.equal(mod(x, wide[..., ::2]), yg)
    assert torch.equal(x, keep_x) and torch.equal(guide, keep_g)
    with pytest.raises(ValueError, match="broadcast"):
        mod(x.expand(-1, 2, -1, -1), guide)
    with pytest.raises(ValueError, match="broadcast"):
        mod(x, guide[..., :36, :])
    for shape in ((0, 1, 8, 8), (2, 0, 8, 8), (2, 1, 0, 8)):
        e = mod(torch.zeros(shape, device=DEV))
        assert e.shape == shape and e.numel() == 0


# ---------------------------------------------------------------------------------------- serving hooks
def _serving():
    if "serving" not in _cache:
        import hiseg
        m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))).eval().to(DEV)
        hiseg.set_compute_dtype(m, torch.bfloat16)
        batches = []
        for k in range(3):
            images = torch.from_numpy(filler.uniform(500 + k, (2, 3, 96, 128))).to(DEV)
            rois = torch.from_numpy(filler.box_rois(600 + k, 2, 3)).to(DEV)
            batches.append((images, rois))
        with torch.no_grad():
            plain = [hiseg.RGBHierarchicalExportWrapper(m)(i, r) for i, r in batches]
        _cache["serving"] = (m, batches, plain)
    return _cache["serving"]


def _hooks():
    import hiseg
    return hiseg.EdgePreservingFilter().to(DEV), hiseg.BinaryMaskEdgeSmoothing().to(DEV)


def test_wrapper_applies_the_hooks_to_its_outputs():
    import hiseg
    from hiseg import engine
    m, batches, plain = _serving()
    bp, ip = _hooks()
    w = hiseg.RGBHierarchicalExportWrapper(m, binary_post=bp, instance_post=ip)
    with torch.no_grad():
        for (images, rois), (inst0, binary0) in zip(batches, plain):
            inst, binary = w(images, rois)
            assert inst.shape == inst0.shape and binary.shape == binary0.shape
            assert torch.equal(inst, ip(inst0)) and torch.equal(binary, bp(binary0))
        assert not torch.equal(binary, binary0)      # the filter did something
        # hooks None: the outputs of the contract as they were
        images, rois = batches[0]
        inst1, binary1 = engine.export_forward(m, images, rois, 0)
        assert torch.equal(plain[0][0], inst1) and torch.equal(plain[0][1], binary1)


@pytest.mark.parametrize("gate", (False, True))
def test_stream_pipelined_export_runs_the_hooks_on_the_producing_streams(gate):
    import hiseg
    m, batches, plain = _serving()
    bp, ip = _hooks()
    kw = dict(gate=True, gate_min_gflop=0.05) if gate else {}
    with torch.no_grad():
        w = hiseg.RGBHierarchicalExportWrapper(m, binary_post=bp, instance_post=ip)
        serial = [w(i, r) for i, r in batches]
        piped = hiseg.StreamPipelinedExport(w, **kw).run(batches)
        none = hiseg.StreamPipelinedExport(hiseg.RGBHierarchicalExportWrapper(m), **kw).run(batches)
    torch.cuda.synchronize()
    assert len(piped) == len(none) == 3
    for (a, b), (c, d), (e, f), (p, q) in zip(serial, piped, none, plain):
        assert torch.equal(a, c) and torch.equal(b, d)
        assert torch.equal(e, p) and torch.equal(f, q)
