"""The directional, adaptive and optimized edge-smoothing filters on the GPU (hiseg.postprocess over
hiseg_dir_edge_smooth_fwd / hiseg_adaptive_edge_smooth_fwd / hiseg_opt_edge_smooth_fwd) against the reference's own
classes run on the CPU (tests/golden/edge_variants.npz, written by gen_edge_variants_golden.py, which explains the
cases, the near sets and the float16 margin).

Per case: the blend before the last threshold within 1e-4 * max(1, |ref|) of the reference's at every pixel, and
the 0/1 output equal to the reference's at every pixel outside the stored near set.  The float16 cases compare the
blend (f32 arithmetic on the float16 input) with the reference's f32 blend of that input, and the decision with the
reference's half-precision run outside |blend - 0.5| <= measured margin + 1e-4.
"""
import numpy as np
import pytest
import torch

import filler
import gen_edge_variants_golden as G
from helpers import b0_kwargs, hiseg_kwargs, load

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_BAR = 1e-4

_cache = {}


def _gold():
    if "npz" not in _cache:
        _cache["npz"] = dict(load("edge_variants"))
    return _cache["npz"]


def _case(filt, kind, name, it):
    """Input planes (float16 for opt16) and the adaptive parameters [3, B] of a recorded case, on the GPU."""
    gold, key, shape = _gold(), G.case_key(filt, kind, name, it), G.SHAPES[name]
    if kind == "bin":
        x = torch.from_numpy(G.unpack(gold[f"{key}/x"], shape).astype(np.float32))
    else:
        x = torch.from_numpy(G.soft_input(int(gold[f"{key}/seed"]), shape))
    x = x.to(DEV)
    params = torch.from_numpy(gold[f"{key}/params"]).to(DEV) if filt == "adaptive" else None
    return (x.half() if filt == "opt16" else x), params


def _op(filt, x, params, it, tiled=False):
    """(0/1 planes, blend) straight from hiseg.ops."""
    from hiseg import ops
    if filt == "dir":
        return ops.dir_edge_smooth(x, it, return_soft=True, _force_tiled=tiled)
    if filt == "adaptive":
        return ops.adaptive_edge_smooth(x, params[0], params[1], params[2], it, return_soft=True, _force_tiled=tiled)
    return ops.opt_edge_smooth(x, it, return_soft=True, _force_tiled=tiled)


def _module(filt):
    import hiseg
    if filt not in _cache:
        _cache[filt] = {"dir": hiseg.DirectionalEdgeSmoothing, "adaptive": hiseg.AdaptiveEdgeSmoothing,
                        "opt": lambda: hiseg.OptimizedEdgeSmoothing(use_fp16=False),
                        "opt16": hiseg.OptimizedEdgeSmoothing}[filt]().to(DEV).eval()
    return _cache[filt]


def _call_module(filt, x, params, it):
    mod = _module(filt)
    if filt == "adaptive":    # [B, 1] tensors, as the reference takes them
        return mod(x, *(p.view(-1, 1) for p in params), iterations=it, return_soft=True)
    return mod(x, iterations=it, return_soft=True)


@pytest.mark.parametrize("filt", G.FILTERS)
def test_every_case_matches_the_reference(filt):
    gold = _gold()
    failed = []
    for f, kind, name, it in G.cases():
        if f != filt:
            continue
        key, shape = G.case_key(f, kind, name, it), G.SHAPES[name]
        x, params = _case(f, kind, name, it)
        out, soft = _call_module(f, x, params, it)
        assert out.shape == shape and soft.shape == shape and soft.dtype == torch.float32
        assert out.dtype == (torch.float16 if filt == "opt16" else torch.float32)
        got = out.float().cpu().numpy()
        assert set(np.unique(got)) <= {0.0, 1.0}, key
        near = G.unpack(gold[f"{key}/near"], shape)
        want = G.unpack(gold[f"{key}/out"], shape)
        bad = int(((got > 0.5) != want)[~near].sum())
        got_soft = soft.cpu().numpy()
        if f"{key}/blend" in gold:
            ref = gold[f"{key}/blend"]
        else:      # the 128x160 / 128x161 pair: the blend on every 8th row and the last
            ref, got_soft = gold[f"{key}/blend_rows"], got_soft[:, :, G.blend_rows(shape[2])]
        err = float((np.abs(got_soft - ref) / np.maximum(1.0, np.abs(ref))).max())
        print(f"{key}: {bad} of {want.size - int(near.sum())} decisions differ, {int(near.sum())} near, "
              f"blend error {err:.3e}")
        if bad or not err <= F32_BAR:
            failed.append((key, bad, err))
    assert not failed, failed


@pytest.mark.parametrize("filt", G.FILTERS)
def test_resident_and_tiled_forms_give_the_same_bits(filt):
    """force_tiled against the default form at every recorded input: planes smaller than a tile, 65x70 (2 x 2
    tiles) and 128x160 (the largest resident plane, 2 x 3 tiles); with 3 iterations the tiled halo is 6."""
    for f, kind, name, it in G.cases():
        if f != filt or name == "128x161":      # 128x161 is tiled either way
            continue
        x, params = _case(f, kind, name, it)
        a, sa = _op(f, x, params, it)
        b, sb = _op(f, x, params, it, tiled=True)
        assert torch.equal(a, b) and torch.equal(sa, sb), G.case_key(f, kind, name, it)


@pytest.mark.parametrize("filt", G.FILTERS)
def test_iterations_in_one_launch_equal_single_launches(filt):
    """On the input of every recorded 1-iteration case (every shape, both kinds), in both forms."""
    for name in G.SHAPES:
        for kind in ("bin", "soft"):
            x, params = _case(filt, kind, name, 1)
            y = x
            for _ in range(3):
                y, soft = _op(filt, y, params, 1)
            for tiled in (False, True):
                one, soft_one = _op(filt, x, params, 3, tiled=tiled)
                assert torch.equal(one, y) and torch.equal(soft_one, soft), (filt, name, kind, tiled)
    # more iterations than one tiled launch holds (16 of radius 2): split into launches, the same bits
    x, params = _case(filt, "bin", "65x70", 1)
    a, sa = _op(filt, x, params, 19)
    b, sb = _op(filt, x, params, 19, tiled=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    c, sc = _op(filt, _op(filt, x, params, 16)[0], params, 3)
    assert torch.equal(a, c) and torch.equal(sa, sc)


def test_adaptive_parameter_forms_agree():
    """param_stride 0 (one element for every plane) against the same value repeated per plane; the reference's
    [B, 1] per-image form on a multi-channel mask; parameters given at construction."""
    import hiseg
    from hiseg import ops
    x = torch.from_numpy(G.soft_input(5, (3, 2, 37, 41))).to(DEV)
    one = [torch.tensor([v], device=DEV) for v in (2.5, 1.3, 0.45)]
    each = [p.repeat(6) for p in one]
    for tiled in (False, True):
        a = ops.adaptive_edge_smooth(x, *one, 2, return_soft=True, _force_tiled=tiled)
        b = ops.adaptive_edge_smooth(x, *each, 2, return_soft=True, _force_tiled=tiled)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    mixed = ops.adaptive_edge_smooth(x, one[0], each[1], one[2].view(1, 1), 2)
    assert torch.equal(mixed, a[0])
    hook = hiseg.AdaptiveEdgeSmoothing(2.5, 1.3, 0.45).to(DEV)
    assert hook.default_blur_strength.is_cuda and torch.equal(hook(x, iterations=2), a[0])
    # one value per image: plane (b, c) uses element b
    per_image = torch.from_numpy(G.adaptive_params(11, 3)).to(DEV)
    mod = hiseg.AdaptiveEdgeSmoothing().to(DEV)
    got = mod(x, *(p.view(3, 1) for p in per_image))
    for b in range(3):
        for c in range(2):
            alone = mod(x[b:b + 1, c:c + 1].contiguous(), *(p[b].view(1, 1) for p in per_image))
            assert torch.equal(got[b:b + 1, c:c + 1], alone), (b, c)
    assert len({float(v) for v in per_image[2]}) == 3 and not torch.equal(got[0], got[1])


@pytest.mark.parametrize("filt", G.FILTERS)
def test_odd_plane_counts(filt):
    """37 planes (a prime: no grid shape divides it) in one call against each plane on its own, in both forms: 37
    workgroups resident, 37 x 2 tiles tiled."""
    x = torch.from_numpy(G.soft_input(21, (37, 1, 9, 70))).to(DEV)
    x[::2] = (x[::2] > 0.5).float()
    params = torch.from_numpy(G.adaptive_params(22, 37)).to(DEV) if filt == "adaptive" else None
    x = x.half() if filt == "opt16" else x
    for tiled in (False, True):
        out, soft = _op(filt, x, params, 2, tiled=tiled)
        for p in (0, 1, 17, 35, 36):
            o1, s1 = _op(filt, x[p:p + 1].contiguous(), None if params is None else params[:, p:p + 1].contiguous(), 2,
                         tiled=tiled)
            assert torch.equal(out[p:p + 1], o1) and torch.equal(soft[p:p + 1], s1), (filt, tiled, p)


def test_module_surface_on_the_gpu():
    import hiseg
    x = torch.from_numpy(G.soft_input(31, (2, 3, 20, 24))).to(DEV)
    keep = x.clone()
    opt16, opt32, dirm = _module("opt16"), _module("opt"), _module("dir")
    y16 = opt16(x)
    assert y16.dtype == torch.float16 and torch.equal(y16, opt16(x.half()))      # the reference's mask.half()
    from hiseg import ops
    big = torch.from_numpy(G.soft_input(32, (2, 1, 65, 70))).to(DEV)             # rounded by the kernel as it loads,
    for tiled in (False, True):                                                  # also across launches (16 + 3)
        for it in (1, 19):
            a = ops.opt_edge_smooth(big, it, to_fp16=True, return_soft=True, _force_tiled=tiled)
            b = ops.opt_edge_smooth(big.half(), it, return_soft=True, _force_tiled=tiled)
            assert a[0].dtype == torch.float16 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert opt32(x).dtype == torch.float32 and dirm(x).dtype == torch.float32
    assert torch.equal(opt32(x.half().float()).half(), y16)                      # f32 arithmetic on the f16 values
    out, soft = dirm(x, iterations=2, return_soft=True)
    assert torch.equal(out, dirm(dirm(x))) and torch.equal(out, (soft > 0.5).float())
    wide = torch.zeros(2, 3, 20, 48, device=DEV)
    wide[..., ::2] = x
    assert torch.equal(dirm(wide[..., ::2]), dirm(x))                            # non-contiguous input
    assert torch.equal(x, keep)
    for m in (dirm, opt16, opt32, hiseg.AdaptiveEdgeSmoothing(3.0, 1.0, 0.5).to(DEV)):
        for shape in ((0, 1, 8, 8), (2, 0, 8, 8), (2, 1, 0, 8)):
            e = m(torch.zeros(shape, device=DEV))
            assert e.shape == shape and e.numel() == 0


# ---------------------------------------------------------------------------------------- serving hooks
def _hooks():
    import hiseg
    return {"dir": hiseg.DirectionalEdgeSmoothing().to(DEV), "adaptive": hiseg.AdaptiveEdgeSmoothing(2.0, 1.0, 0.45).to(DEV),
            "opt": hiseg.OptimizedEdgeSmoothing(use_fp16=False).to(DEV), "opt16": hiseg.OptimizedEdgeSmoothing().to(DEV)}


def _serving():
    if "serving" not in _cache:
        import hiseg
        m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))).eval().to(DEV)
        hiseg.set_compute_dtype(m, torch.bfloat16)
        batches = []
        for k in range(2):
            images = torch.from_numpy(filler.uniform(700 + k, (2, 3, 96, 128))).to(DEV)
            rois = torch.tensor([[0, .10, .10, .40, .90], [1, .35, .15, .80, .95], [0, .55, .05 + .1 * k, .95, .70]],
                                dtype=torch.float32, device=DEV)
            batches.append((images, rois))
        with torch.no_grad():
            plain = [hiseg.RGBHierarchicalExportWrapper(m)(i, r) for i, r in batches]
        _cache["serving"] = (m, batches, plain)
    return _cache["serving"]


def test_filters_serve_as_wrapper_and_pipeline_hooks():
    """Each module as instance_post and as binary_post of the export wrapper (2 images of 96x128, 3 ROIs): the bits
    of the module applied to the wrapper's unfiltered outputs, also under StreamPipelinedExport, where the hook
    launches on the stream that produced its masks."""
    import hiseg
    m, batches, plain = _serving()
    assert plain[0][0].shape[0] == 3 and plain[0][1].shape == (2, 1, 96, 128)
    hooks = _hooks()
    with torch.no_grad():
        for name, hook in hooks.items():
            w = hiseg.RGBHierarchicalExportWrapper(m, binary_post=hook, instance_post=hook)
            serial = [w(i, r) for i, r in batches]
            piped = hiseg.StreamPipelinedExport(w).run(batches)
            torch.cuda.synchronize()
            for (inst, binary), (pi, pb), (inst0, binary0) in zip(serial, piped, plain):
                assert inst.shape == inst0.shape and binary.shape == binary0.shape
                assert torch.equal(inst, hook(inst0)) and torch.equal(binary, hook(binary0)), name
                assert torch.equal(pi, inst) and torch.equal(pb, binary), name
            assert set(np.unique(binary.float().cpu().numpy())) <= {0.0, 1.0}


@pytest.mark.parametrize("filt", G.FILTERS)
def test_graph_capture_replays_bit_identically(filt):
    """One call captured in a HIP graph: the replay equals the eager call, also after the input -- and, for the
    adaptive filter, the device-side parameters -- changed in place (no host read of either)."""
    x0, params = _case(filt, "soft", "65x70", 1)
    x1, _ = _case(filt, "bin", "65x70", 1)
    x = x0.clone()
    eager0, eager1 = _op(filt, x0, params, 2), _op(filt, x1, params, 2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):       # warm-up on the capture stream's side: the LDS attribute is set here
        _op(filt, x, params, 2)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, soft = _op(filt, x, params, 2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0[0]) and torch.equal(soft, eager0[1])
    x.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager1[0]) and torch.equal(soft, eager1[1])
    if filt == "adaptive":
        new = torch.from_numpy(G.adaptive_params(99, 2)).to(DEV)
        want = _op(filt, x1, new, 2)
        params.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[0]) and torch.equal(soft, want[1]) and not torch.equal(out, eager1[0])
