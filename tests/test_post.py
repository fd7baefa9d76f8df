"""Mask post-processing without a GPU: the C ABI of include/hiseg_post.h, the modules' state_dict against the
reference's (tests/golden/state_keys_post.json, post.npz from gen_post_golden.py) and argument checking."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_abi import header_functions

ENTRY_POINTS = ("hiseg_edge_smooth_fwd", "hiseg_class_edge_smooth_fwd", "hiseg_var_gated_blur_fwd",
                "hiseg_morph_bilateral_fwd", "hiseg_bilateral_fwd")
BAD_ARG = -1


def _configs():
    with open(os.path.join(GOLDEN, "state_keys_post.json")) as f:
        return {k: v for k, v in json.load(f).items() if not k.startswith("_")}


def test_header_declares_and_library_binds_the_entry_points():
    from hiseg import _lib as L
    declared = header_functions(["hiseg_post.h"])
    lib = L.lib()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.EXPORTED, name
    assert set(declared) <= set(L.EXPORTED)


def test_state_dict_keys_shapes_and_buffer_values_match_the_reference():
    import hiseg
    gold = np.load(os.path.join(GOLDEN, "post.npz"))
    cfgs = _configs()
    assert {c["class"] for c in cfgs.values()} == {
        "BinaryMaskEdgeSmoothing", "BilateralFilter", "FastBilateralFilter", "BinaryMaskBilateralFilter",
        "MorphologicalBilateralFilter"}
    for name, cfg in cfgs.items():
        sd = getattr(hiseg, cfg["class"])(**cfg["kwargs"]).state_dict()
        assert {k: list(v.shape) for k, v in sd.items()} == cfg["keys"], name
        for k, v in sd.items():
            assert v.dtype == torch.float32
            np.testing.assert_allclose(v.numpy(), gold[f"buf/{name}/{k}"], rtol=0, atol=1e-7, err_msg=f"{name} {k}")
    # the multi-class helper holds a BinaryMaskEdgeSmoothing as `smoother`, as the reference does
    mc = hiseg.MultiClassEdgeSmoothing(threshold=0.4, blur_strength=1.5, iterations=3, device="cpu")
    assert isinstance(mc.smoother, hiseg.BinaryMaskEdgeSmoothing) and not mc.smoother.training
    assert (mc.smoother.threshold, mc.smoother.blur_strength, mc.iterations) == (0.4, 1.5, 3)


def test_cpu_tensors_are_refused():
    import hiseg
    x = torch.zeros(1, 1, 8, 8)
    for mod in (hiseg.BinaryMaskEdgeSmoothing(), hiseg.BilateralFilter(), hiseg.FastBilateralFilter(),
                hiseg.BinaryMaskBilateralFilter(), hiseg.MorphologicalBilateralFilter()):
        with pytest.raises(RuntimeError, match="GPU only"):
            mod(x)
    mc = hiseg.MultiClassEdgeSmoothing(device="cpu")
    for pred in (torch.zeros(1, 3, 8, 8), np.zeros((2, 8, 8), np.float32)):
        with pytest.raises(RuntimeError, match="GPU only"):
            mc.smooth_predictions(pred)
    with pytest.raises(RuntimeError, match="GPU only"):
        hiseg.apply_edge_smoothing_to_masks(torch.zeros(3, 8, 8), device="cpu")


def test_even_kernel_size_raises():
    import hiseg
    for cls in (hiseg.BilateralFilter, hiseg.FastBilateralFilter, hiseg.BinaryMaskBilateralFilter,
                hiseg.MorphologicalBilateralFilter):
        with pytest.raises(ValueError, match="odd"):
            cls(kernel_size=4)
    with pytest.raises(ValueError, match="odd"):
        hiseg.MorphologicalBilateralFilter(morph_size=2)


def test_bad_arguments_are_refused_without_touching_the_gpu():
    from hiseg import _lib as L
    lib = L.lib()
    fake = 1 << 20   # never dereferenced: every call below is refused before a launch
    err = lib.hiseg_last_error_string

    assert lib.hiseg_edge_smooth_fwd(None, fake, 1, 8, 8, 0.5, 3.0, 1, 0, 0, None) == BAD_ARG
    assert b"null" in err()
    assert lib.hiseg_edge_smooth_fwd(fake, fake, 1, 8, 8, 0.5, 3.0, 0, 0, 0, None) == BAD_ARG
    assert b"iterations" in err()
    assert lib.hiseg_class_edge_smooth_fwd(fake, None, 1, 8, 8, 0.5, 3.0, 1, 0, None) == BAD_ARG
    assert b"null" in err()
    assert lib.hiseg_var_gated_blur_fwd(fake, fake, 1, 8, 8, 4, 1.0, 10.0, 1, 1, 0.5, 1, 0, None) == BAD_ARG
    assert b"kernel_size 4" in err()
    assert lib.hiseg_var_gated_blur_fwd(None, fake, 1, 8, 8, 5, 1.0, 10.0, 1, 1, 0.5, 1, 0, None) == BAD_ARG
    assert b"null" in err()
    assert lib.hiseg_var_gated_blur_fwd(fake, fake, 1, 8, 8, 11, 1.0, 10.0, 1, 1, 0.5, 1, 0, None) == BAD_ARG
    assert lib.hiseg_morph_bilateral_fwd(fake, fake, 1, 8, 8, 4, 1.0, 3, 0, None) == BAD_ARG
    assert b"kernel_size 4" in err()
    assert lib.hiseg_morph_bilateral_fwd(fake, fake, 1, 8, 8, 5, 1.0, 4, 0, None) == BAD_ARG
    assert b"morph_size 4" in err()
    assert lib.hiseg_morph_bilateral_fwd(fake, None, 1, 8, 8, 5, 1.0, 3, 0, None) == BAD_ARG
    assert lib.hiseg_bilateral_fwd(fake, fake, 1, 8, 8, 4, 1.0, 0.1, None) == BAD_ARG
    assert b"kernel_size 4" in err()
    assert lib.hiseg_bilateral_fwd(None, fake, 1, 8, 8, 5, 1.0, 0.1, None) == BAD_ARG
    # reflect padding needs H, W > kernel_size / 2 (F.pad refuses it too)
    assert lib.hiseg_bilateral_fwd(fake, fake, 1, 2, 3, 5, 1.0, 0.1, None) == BAD_ARG
    assert b"reflect" in err()
    # the tiled form holds a halo of at most 32 pixels: 200 x 264 planes, 9 iterations of radius 4
    assert lib.hiseg_var_gated_blur_fwd(fake, fake, 1, 200, 264, 9, 1.0, 10.0, 1, 1, 0.5, 9, 0, None) == BAD_ARG
    assert b"halo" in err()
    # empty inputs are fine and launch nothing (an empty tensor has no address)
    assert lib.hiseg_edge_smooth_fwd(None, None, 0, 8, 8, 0.5, 3.0, 1, 0, 0, None) == 0
    assert lib.hiseg_var_gated_blur_fwd(None, None, 4, 0, 8, 5, 1.0, 10.0, 1, 1, 0.5, 1, 0, None) == 0
    assert lib.hiseg_morph_bilateral_fwd(None, None, 0, 8, 8, 5, 1.0, 3, 0, None) == 0
    assert lib.hiseg_bilateral_fwd(None, None, 0, 8, 8, 5, 1.0, 0.1, None) == 0


def test_iterations_per_launch_follow_the_lds_limit():
    """hiseg_post_max_iterations (host only): planes of up to 20480 pixels are LDS resident (any iteration count in
    one launch); larger ones, or any with the tiled form forced, get 32 / radius iterations per launch."""
    from hiseg import _lib as L
    from hiseg import ops
    f = L.lib().hiseg_post_max_iterations
    big = 0x7fffffff
    assert f(48, 64, 1, 0) == big and f(96, 128, 3, 0) == big and f(128, 160, 4, 0) == big
    assert f(200, 264, 1, 0) == 32 and f(200, 264, 3, 0) == 10 and f(480, 640, 4, 0) == 8
    assert f(129, 160, 1, 0) == 32          # 20640 pixels: just past the limit
    assert f(48, 64, 1, 1) == 32 and f(48, 64, 2, 1) == 16
    assert ops._post_chunks(5, 48, 64, 3, False) == [5]
    assert ops._post_chunks(25, 200, 264, 3, False) == [10, 10, 5]
    assert ops._post_chunks(3, 48, 64, 4, True) == [3]
    with pytest.raises(ValueError):
        ops._post_chunks(0, 48, 64, 1, False)
