"""The directional, adaptive and optimized edge-smoothing filters without a GPU: the public surface against the
reference's (tests/golden/edge_variants.npz, written by gen_edge_variants_golden.py), argument checking of the Python
layers and of the C entry points, and the invariants of the fixture itself."""
import inspect
import os

import numpy as np
import pytest
import torch

import gen_edge_variants_golden as G
from conftest import GOLDEN
from test_abi import header_functions

ENTRY_POINTS = ("hiseg_dir_edge_smooth_fwd", "hiseg_adaptive_edge_smooth_fwd", "hiseg_opt_edge_smooth_fwd")
BAD_ARG, BAD_DTYPE = -1, -3
_cache = {}


def _gold():
    if not _cache:
        _cache.update(np.load(os.path.join(GOLDEN, "edge_variants.npz")))
    return _cache


def test_public_names_are_exported():
    import hiseg
    for name in G.CLASSES.values():
        assert hasattr(hiseg, name) and name in hiseg.postprocess.__all__
        assert issubclass(getattr(hiseg, name), torch.nn.Module)


def test_constructor_signatures_are_the_reference_ones():
    import hiseg

    def params(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    assert params(hiseg.DirectionalEdgeSmoothing) == [("num_directions", 4)]
    assert params(hiseg.OptimizedEdgeSmoothing) == [("use_fp16", True)]
    # the reference takes no argument; the three optional ones make the module a one-argument hook
    assert params(hiseg.AdaptiveEdgeSmoothing) == [("blur_strength", None), ("edge_sensitivity", None),
                                                   ("final_threshold", None)]
    assert hiseg.DirectionalEdgeSmoothing(num_directions=9).num_directions == 9     # stored, never read
    assert hiseg.OptimizedEdgeSmoothing().use_fp16 is True and hiseg.OptimizedEdgeSmoothing(False).use_fp16 is False
    fwd = list(inspect.signature(hiseg.AdaptiveEdgeSmoothing.forward).parameters)
    assert fwd[:5] == ["self", "mask", "blur_strength", "edge_sensitivity", "final_threshold"]
    for cls in G.CLASSES.values():
        sig = inspect.signature(getattr(hiseg, cls).forward).parameters
        assert sig["iterations"].default == 1 and sig["return_soft"].default is False


@pytest.mark.parametrize("cls", sorted(G.CLASSES.values()))
def test_state_dict_is_the_reference_one_and_loads_strictly(cls):
    import hiseg
    gold = _gold()
    want = [str(s) for s in gold[f"keys/{cls}"]]
    m = getattr(hiseg, cls)()
    sd = m.state_dict()
    assert [k + "|" + ",".join(str(d) for d in v.shape) for k, v in sd.items()] == want
    ref_sd = {k.split("|")[0]: torch.from_numpy(gold[f"buf/{cls}/{k.split('|')[0]}"]) for k in want}
    for k, v in sd.items():
        assert v.dtype == torch.float32 and torch.equal(v, ref_sd[k]), k
    res = getattr(hiseg, cls)().load_state_dict(ref_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # the kernels use the fixed taps: a checkpoint with other values is refused, not ignored
    first = want[0].split("|")[0]
    bad = dict(ref_sd)
    bad[first] = ref_sd[first] * 2
    with pytest.raises(ValueError, match="differs"):
        getattr(hiseg, cls)().load_state_dict(bad, strict=True)


def test_half_checkpoint_of_the_optimized_filter_loads():
    import hiseg
    gold = _gold()
    sd = {k.split("|")[0]: torch.from_numpy(gold[f"buf/OptimizedEdgeSmoothing/{k.split('|')[0]}"]).half()
          for k in (str(s) for s in gold["keys/OptimizedEdgeSmoothing"])}
    hiseg.OptimizedEdgeSmoothing().load_state_dict(sd, strict=True)    # every tap is exact in float16


def test_adaptive_construction_parameters_stay_out_of_the_state_dict():
    import hiseg
    m = hiseg.AdaptiveEdgeSmoothing(3.0, 1.0, torch.tensor([0.5]))
    assert list(m.state_dict()) == ["laplacian_kernel"]
    assert m.default_blur_strength.dtype == torch.float32 and float(m.default_blur_strength) == 3.0
    assert float(m.default_final_threshold) == 0.5
    with pytest.raises(ValueError, match="float32"):
        hiseg.AdaptiveEdgeSmoothing(torch.tensor([1]), 1.0, 0.5)


def test_cpu_tensors_are_refused():
    import hiseg
    from hiseg import ops
    x = torch.zeros(1, 1, 8, 8)
    p = torch.ones(1, 1)
    for call in (lambda: hiseg.DirectionalEdgeSmoothing()(x), lambda: hiseg.OptimizedEdgeSmoothing()(x),
                 lambda: hiseg.OptimizedEdgeSmoothing(False)(x), lambda: hiseg.AdaptiveEdgeSmoothing()(x, p, p, p),
                 lambda: hiseg.AdaptiveEdgeSmoothing(3.0, 1.0, 0.5)(x), lambda: ops.dir_edge_smooth(x),
                 lambda: ops.opt_edge_smooth(x.half()), lambda: ops.adaptive_edge_smooth(x, p, p, p)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_bad_rank_and_dtype_are_refused():
    import hiseg
    p = torch.ones(1, 1)
    mods = (hiseg.DirectionalEdgeSmoothing(), hiseg.OptimizedEdgeSmoothing(), hiseg.OptimizedEdgeSmoothing(False),
            hiseg.AdaptiveEdgeSmoothing(3.0, 1.0, 0.5))
    for m in mods:
        for bad in (torch.zeros(8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 1, 1, 8, 8)):
            with pytest.raises(ValueError, match="B, C, H, W"):
                m(bad)
        for dt in (torch.float64, torch.bfloat16, torch.int64, torch.bool):
            with pytest.raises(ValueError, match="expected a mask of"):
                m(torch.zeros(1, 1, 8, 8, dtype=dt))
    for m in (mods[0], mods[2], mods[3]):      # float16 planes are the optimized filter's use_fp16 path only
        with pytest.raises(ValueError, match="expected a mask of"):
            m(torch.zeros(1, 1, 8, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="neither"):
        hiseg.AdaptiveEdgeSmoothing()(torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError, match="neither"):
        hiseg.AdaptiveEdgeSmoothing(blur_strength=3.0)(torch.zeros(1, 1, 8, 8), edge_sensitivity=p)


def test_entry_points_are_declared_and_bound():
    from hiseg import _lib as L
    declared = header_functions(["hiseg_post.h"])
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(L.lib(), name) and name in L.EXPORTED


def test_bad_arguments_are_refused_without_touching_the_gpu():
    from hiseg import _lib as L
    lib = L.lib()
    err = lib.hiseg_last_error_string
    fake, fake2, fake3 = 1 << 20, 1 << 21, 1 << 22    # never dereferenced: every call below returns before a launch
    d, a, o = lib.hiseg_dir_edge_smooth_fwd, lib.hiseg_adaptive_edge_smooth_fwd, lib.hiseg_opt_edge_smooth_fwd
    # zero-size problems launch nothing
    assert d(None, None, None, 0, 8, 8, 1, 0, None) == 0
    assert a(None, None, None, 2, 0, 8, None, None, None, 0, 1, 0, None) == 0
    assert o(L.HISEG_POST_F16, None, None, None, 2, 8, 0, 1, 1, None) == 0
    for it in (0, -1):
        assert d(fake, fake2, None, 1, 8, 8, it, 0, None) == BAD_ARG and b"iterations" in err()
        assert a(fake, fake2, None, 1, 8, 8, fake3, fake3, fake3, 0, it, 0, None) == BAD_ARG
        assert o(L.HISEG_POST_F32, fake, fake2, None, 1, 8, 8, it, 0, None) == BAD_ARG
    assert d(fake, None, None, 1, 8, 8, 1, 0, None) == BAD_ARG and b"null" in err()
    assert d(fake, fake, None, 1, 8, 8, 1, 0, None) == BAD_ARG and b"alias" in err()
    assert d(fake, fake2, fake2, 1, 8, 8, 1, 0, None) == BAD_ARG and b"alias" in err()
    assert a(fake, fake2, None, 1, 8, 8, fake3, None, fake3, 1, 1, 0, None) == BAD_ARG and b"parameter" in err()
    assert a(fake, fake2, None, 1, 8, 8, fake3, fake3, fake3, -1, 1, 0, None) == BAD_ARG and b"param_stride" in err()
    assert o(L.HISEG_POST_F32_TO_F16, fake, fake2, None, 1, 8, 8, 0, 0, None) == BAD_ARG and b"iterations" in err()
    for dtype in (1, 4, -1):     # bf16 planes are not built
        assert o(dtype, fake, fake2, None, 1, 8, 8, 1, 0, None) == BAD_DTYPE and b"dtype" in err()
    # the tiled form holds a halo of 32 = 16 iterations of radius 2; the resident form any number
    assert d(fake, fake2, None, 1, 8, 8, 17, 1, None) == BAD_ARG and b"halo" in err()
    assert d(fake, fake2, None, 1, 128, 161, 17, 0, None) == BAD_ARG and b"halo" in err()
    assert lib.hiseg_post_max_iterations(128, 161, 2, 0) == 16 and lib.hiseg_post_max_iterations(128, 160, 2, 1) == 16
    assert lib.hiseg_post_max_iterations(128, 160, 2, 0) == 0x7fffffff


def test_fixture_holds_every_case_and_its_invariants():
    gold = _gold()
    cases = G.cases()
    # 4 filters x 8 shapes x 2 kinds x 2 iteration counts, less the 7 soft 3-iteration cases that have no seed
    assert len(cases) == 4 * 8 * 2 * 2 - 7 == 121 and len(G.ABSENT) == 7
    for filt, kind, name, it in G.ABSENT:
        assert kind == "soft" and it == 3 and (name in G.PACKED_ONLY or (filt, name) == ("opt16", "65x70"))
        assert filt != "adaptive"
    for shape in G.SHAPES.values():
        assert shape[1] == 1 and shape[0] >= 2      # the adaptive parameters differ between the planes of a call
    for filt, kind, name, it in cases:
        key = G.case_key(filt, kind, name, it)
        shape = G.SHAPES[name]
        px = int(np.prod(shape))
        near = G.unpack(gold[f"{key}/near"], shape)
        cap = G.NEAR_CAP_F16 if filt == "opt16" else G.NEAR_CAP
        assert near.mean() <= cap, (key, near.mean())
        assert gold[f"{key}/out"].size == (px + 7) // 8
        assert (f"{key}/blend" in gold) == (name not in G.PACKED_ONLY), key
        assert (f"{key}/blend_rows" in gold) == (name in G.PACKED_ONLY), key
        thr = gold[f"{key}/params"][2].reshape(-1, 1, 1, 1) if filt == "adaptive" else 0.5
        if name in G.PACKED_ONLY:     # the blend on every 8th row and the last: the same invariants on those rows
            rows = G.blend_rows(shape[2])
            assert rows[0] == 0 and rows[-1] == shape[2] - 1 and len(rows) == 17
            part = gold[f"{key}/blend_rows"]
            assert part.shape == shape[:2] + (17, shape[3]) and part.dtype == np.float32
            agree = (part > thr) == G.unpack(gold[f"{key}/out"], shape)[:, :, rows]
            assert agree[~near[:, :, rows]].all() if filt == "opt16" else agree.all(), key
        if f"{key}/blend" in gold:
            blend = gold[f"{key}/blend"]
            assert blend.shape == shape and blend.dtype == np.float32
            out = G.unpack(gold[f"{key}/out"], shape)
            if filt == "opt16":     # the oracle is the half-precision run: it may differ from the f32 blend inside near
                assert ((blend > thr) == out)[~near].all(), key
                margin = float(gold[f"{key}/margin"])
                assert 0.0 <= margin < 2e-3, (key, margin)
                if kind == "soft":
                    np.testing.assert_array_equal(near, np.abs(blend - 0.5) <= np.float32(margin + G.F32_BAR))
            else:
                np.testing.assert_array_equal(blend > thr, out)
        if kind == "bin":
            x = G.unpack(gold[f"{key}/x"], shape)
            np.testing.assert_array_equal(x, G.binary_input(int(gold[f"{key}/seed"]), shape) > 0.5)
        if filt == "adaptive":
            params = gold[f"{key}/params"]
            assert params.shape == (3, shape[0]) and params.dtype == np.float32
            for row, (lo, hi) in zip(params, G.RANGES.values()):
                assert (row >= lo).all() and (row <= hi).all(), key
                assert len(set(row.tolist())) == shape[0], key
    # 3 iterations: every filter on binary inputs at every shape; on soft maps wherever a clean seed exists
    its3 = {(f, k, n) for f, k, n, it in cases if it == 3}
    for filt in G.FILTERS:
        for name in G.SHAPES:
            assert (filt, "bin", name) in its3
    for filt in ("dir", "adaptive", "opt"):
        assert (filt, "soft", "65x70") in its3
    for name in G.SHAPES:
        assert ("adaptive", "soft", name) in its3
    for name in ("1x1", "1x5", "5x1", "3x3", "7x9"):
        assert ("opt16", "soft", name) in its3


@pytest.mark.parametrize("hook", ("binary_post", "instance_post"))
@pytest.mark.parametrize("cls", sorted(G.CLASSES.values()))
def test_traced_export_refuses_a_wrapper_with_one_of_these_hooks(cls, hook):
    """As for the existing filters (tests/test_guided.py): the hook is a HIP kernel, not a graph of operators."""
    import filler
    import hiseg
    from helpers import b0_kwargs, hiseg_kwargs
    if "model" not in _cache:
        torch.manual_seed(0)
        _cache["model"] = filler.fill_module(hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))).eval()
    post = hiseg.AdaptiveEdgeSmoothing(3.0, 1.0, 0.5) if cls == "AdaptiveEdgeSmoothing" else getattr(hiseg, cls)()
    wrapper = hiseg.RGBHierarchicalExportWrapper(_cache["model"], **{hook: post}).eval()
    images = torch.from_numpy(filler.uniform(41, (2, 3, 96, 128)))
    rois = torch.from_numpy(filler.box_rois(42, 2, 2))
    with pytest.raises(Exception) as info:
        torch.export.export(wrapper, (images, rois))
    chain, e = [], info.value
    while e is not None:
        chain.append(e)
        e = e.__cause__ or e.__context__
    assert any(isinstance(c, NotImplementedError) or "NotImplementedError" in str(c) for c in chain), chain
    assert any(hook in str(c) for c in chain), chain
