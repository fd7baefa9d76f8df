"""Mask post-processing on the GPU (hiseg.postprocess over include/hiseg_post.h) against the reference's own
classes run on the CPU in f32 (tests/golden/post.npz, written by gen_post_golden.py).

Fixtures: tiny 2x1x2x3 (smaller than every kernel), odd 3x1x37x53, roi 2x1x48x64 (LDS-resident form), big
1x1x200x264 = 52800 pixels -- past the resident form's limit of 20480 pixels (160 KB of LDS / two f32 copies), so it
takes 64x64 tiles with a halo in both axes.  Thresholded outputs are compared at every pixel: the generator
asserted that no pre-threshold value (float64) lies within 1e-5 of the threshold, except for edge smoothing on
binary masks, where the f32 rounding of the reference is reproduced exactly (385 pixels of the fixtures blend to
exactly 0.5).  Soft outputs: max |diff| <= 1e-5 on values in [0, 1] ((taps + a few) * 2^-24 ~ 5e-6 for 81 taps).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("tiny", "odd", "roi", "big")
INPUTS = tuple(f"{kind}_{n}" for kind in ("bin", "soft") for n in NAMES)
SOFT_TOL = 1e-5

_cache = {}


def _gold():
    if not _cache:
        _cache["npz"] = dict(np.load(os.path.join(GOLDEN, "post.npz")))
        with open(os.path.join(GOLDEN, "state_keys_post.json")) as f:
            _cache["cfg"] = json.load(f)
    return _cache["npz"], _cache["cfg"]


def _input(name):
    return torch.from_numpy(_gold()[0][f"in/{name}"].astype(np.float32)).to(DEV)


def _module(cfg):
    import hiseg
    c = _gold()[1][cfg]
    return getattr(hiseg, c["class"])(**c["kwargs"]).to(DEV).eval(), c


def _assert_same_mask(got, key, what):
    want = _gold()[0][key]
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, what
    bad = int((got != want.astype(np.float32)).sum())
    print(f"{what}: {bad} of {want.size} pixels differ")
    assert bad == 0, f"{what}: {bad} of {want.size} pixels differ"


@pytest.mark.parametrize("tag", ("def", "alt"))
@pytest.mark.parametrize("name", NAMES)
def test_edge_smoothing_binary_is_bit_identical(name, tag):
    mod, c = _module(f"BinaryMaskEdgeSmoothing/{tag}")
    y = _input(f"bin_{name}")
    for _ in range(c["iterations"]):
        y = mod(y)
    _assert_same_mask(y, f"edge/{tag}/bin_{name}", f"edge {tag} bin_{name}")
    # the same iterations in one launch
    from hiseg import ops
    one = ops.edge_smooth(_input(f"bin_{name}"), mod.threshold, mod.blur_strength, c["iterations"])
    assert torch.equal(one, y)


@pytest.mark.parametrize("tag", ("def", "alt"))
@pytest.mark.parametrize("name", NAMES)
def test_edge_smoothing_soft_matches_at_every_pixel(name, tag):
    mod, c = _module(f"BinaryMaskEdgeSmoothing/{tag}")
    y = _input(f"soft_{name}")
    for _ in range(c["iterations"]):
        y = mod(y)
    _assert_same_mask(y, f"edge/{tag}/soft_{name}", f"edge {tag} soft_{name}")


@pytest.mark.parametrize("cls,short", (("BinaryMaskBilateralFilter", "binbil"), ("MorphologicalBilateralFilter", "morph")))
@pytest.mark.parametrize("tag", ("def", "alt"))
@pytest.mark.parametrize("iname", INPUTS)
def test_thresholded_filters_match_at_every_pixel(iname, tag, cls, short):
    mod, _ = _module(f"{cls}/{tag}")
    _assert_same_mask(mod(_input(iname)), f"{short}/{tag}/{iname}", f"{short} {tag} {iname}")


@pytest.mark.parametrize("tag", ("def", "alt"))
def test_fast_bilateral_within_1e5(tag):
    mod, _ = _module(f"FastBilateralFilter/{tag}")
    gold = _gold()[0]
    seen = 0
    for iname in INPUTS:
        key = f"fast/{tag}/{iname}"
        if key not in gold:      # `big` is recorded for the defaults on the soft input only (fixture size)
            continue
        got = mod(_input(iname)).cpu().numpy()
        err = float(np.abs(got - gold[key]).max())
        print(f"fast {tag} {iname}: max |diff| {err:.3e}")
        assert got.shape == gold[key].shape and err <= SOFT_TOL, (iname, err)
        seen += 1
    assert seen == (7 if tag == "def" else 6)


@pytest.mark.parametrize("tag", ("k5", "k3"))
def test_bilateral_within_1e5(tag):
    mod, _ = _module(f"BilateralFilter/{tag}")
    gold = _gold()[0]
    got = mod(_input("bil_x")).cpu().numpy()
    err = float(np.abs(got - gold[f"bil/{tag}"]).max())
    print(f"bilateral {tag}: max |diff| {err:.3e}")
    assert got.shape == (2, 2, 9, 11) and err <= SOFT_TOL, err
    # reflect padding is illegal on a plane no larger than the padding, as in F.pad
    from hiseg._lib import HisegError
    with pytest.raises(HisegError, match="reflect"):
        mod(torch.zeros(1, 1, mod.padding, 8, device=DEV))
    assert mod(torch.zeros(1, 1, mod.padding + 1, mod.padding + 1, device=DEV)).abs().max().item() == 0.0


@pytest.mark.parametrize("name,shape", (("mc_a", (2, 3, 37, 53)), ("mc_b", (3, 37, 53))))
def test_multi_class_edge_smoothing(name, shape):
    import hiseg
    gold, cfg = _gold()
    want = gold[f"mc/{name}"].astype(np.float32)
    assert want.shape == shape
    scores = gold[f"in/{name}"]
    mc = hiseg.MultiClassEdgeSmoothing(iterations=cfg["_meta"]["mc_iterations"], device=DEV)
    got = mc.smooth_predictions(torch.from_numpy(scores).to(DEV))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    got_np = mc.smooth_predictions(scores)
    assert isinstance(got_np, np.ndarray) and got_np.dtype == np.float32 and got_np.shape == shape
    np.testing.assert_array_equal(got_np, want)
    got_fn = hiseg.apply_edge_smoothing_to_masks(scores, iterations=cfg["_meta"]["mc_iterations"], device=DEV)
    np.testing.assert_array_equal(got_fn, want)
    if len(shape) == 3:      # (C, H, W) input: the batch dimension is added and squeezed again
        np.testing.assert_array_equal(mc.smooth_predictions(scores[0]), want)


def test_multi_class_ties_and_probability_path():
    """Ties: the first maximum wins, as torch.argmax.  Other class counts: the mask is p > 0.5."""
    import hiseg
    from hiseg import ops
    g = torch.Generator().manual_seed(3)
    s = (torch.round(torch.randn(2, 3, 19, 23, generator=g) * 2) / 2).to(DEV)   # many exact ties
    am = s.argmax(dim=1)
    assert int(((s[:, 0] == s[:, 1]) & (s[:, 0] >= s[:, 2])).sum()) > 20
    onehot = torch.stack([(am == c).float() for c in range(3)], dim=1)
    mc = hiseg.MultiClassEdgeSmoothing(iterations=2, device=DEV)
    assert torch.equal(mc.smooth_predictions(s), ops.edge_smooth(onehot, iterations=2))
    p = torch.rand(2, 4, 19, 23, generator=g).to(DEV)
    p[0, 0, 0, :4] = 0.5     # 0.5 is not > 0.5
    assert torch.equal(mc.smooth_predictions(p), ops.edge_smooth((p > 0.5).float(), iterations=2))


def test_tiled_form_equals_resident_form():
    from hiseg import ops
    for kind in ("bin", "soft"):
        x = _input(f"{kind}_roi")
        for it in (1, 3):
            assert torch.equal(ops.edge_smooth(x, 0.5, 3.0, it), ops.edge_smooth(x, 0.5, 3.0, it, _force_tiled=True))
        s = torch.from_numpy(_gold()[0]["in/mc_a"]).to(DEV)
        assert torch.equal(ops.class_edge_smooth(s, iterations=2), ops.class_edge_smooth(s, iterations=2, _force_tiled=True))
        for k, sig, thr in ((7, 1.5, 0.5), (5, 1.0, None), (9, 2.0, None), (3, 0.8, 0.5)):
            a = ops.var_gated_blur(x, k, sig, 10.0, 2, clamp_input=True, threshold=thr)
            b = ops.var_gated_blur(x, k, sig, 10.0, 2, clamp_input=True, threshold=thr, _force_tiled=True)
            assert torch.equal(a, b), (kind, k)
        for k, m in ((5, 3), (3, 5), (9, 1), (7, 9)):
            assert torch.equal(ops.morph_bilateral(x, k, 1.0, m), ops.morph_bilateral(x, k, 1.0, m, _force_tiled=True)), (k, m)


@pytest.mark.parametrize("name", ("roi", "big"))
def test_iterations_in_one_launch_equal_single_launches(name):
    """The halo and re-padding check: 3 iterations in one launch (halo 3 x radius in the tiled form, the image
    border re-padded at every iteration) are bit-identical to 3 launches of one iteration."""
    from hiseg import ops
    for kind in ("bin", "soft"):
        x = _input(f"{kind}_{name}")
        y = x
        for _ in range(3):
            y = ops.edge_smooth(y, 0.5, 3.0, 1)
        assert torch.equal(ops.edge_smooth(x, 0.5, 3.0, 3), y)
        y = x.clamp(0, 1)
        for _ in range(3):
            y = ops.var_gated_blur(y, 7, 1.5, 10.0, 1)
        assert torch.equal(ops.var_gated_blur(x, 7, 1.5, 10.0, 3, clamp_input=True), y)
        assert torch.equal(ops.var_gated_blur(x, 7, 1.5, 10.0, 3, clamp_input=True, threshold=0.5), (y > 0.5).float())
    # more iterations than one tiled launch holds (32 / radius 4 = 8): split into launches, the same bits
    x = _input(f"soft_{name}")
    many = ops.var_gated_blur(x, 9, 2.0, 10.0, 10, clamp_input=True)
    assert torch.equal(many, ops.var_gated_blur(ops.var_gated_blur(x, 9, 2.0, 10.0, 4, clamp_input=True), 9, 2.0, 10.0, 6))


def test_input_forms_agree_and_input_is_untouched():
    import hiseg
    mod = hiseg.BinaryMaskEdgeSmoothing().to(DEV)
    x4 = _input("bin_odd").reshape(1, 3, 37, 53)
    keep = x4.clone()
    y4 = mod(x4)
    assert y4.shape == x4.shape and y4.dtype == x4.dtype
    y3 = mod(x4[0])
    assert y3.shape == (3, 37, 53) and torch.equal(y3, y4[0])
    y2 = mod(x4[0, 1])
    assert y2.shape == (37, 53) and torch.equal(y2, y4[0, 1])
    assert torch.equal(x4, keep)
    # the input dtype comes back
    for dt in (torch.bool, torch.uint8, torch.float16, torch.int64):
        yd = mod(x4.to(dt))
        assert yd.dtype == dt and torch.equal(yd.float(), y4)
    # a non-contiguous input gives what its contiguous copy gives
    wide = torch.zeros(1, 3, 37, 106, device=DEV)
    wide[..., ::2] = x4
    assert torch.equal(mod(wide[..., ::2]), y4)
    t = x4.permute(0, 1, 3, 2)
    assert not t.is_contiguous() and torch.equal(mod(t), mod(t.contiguous()))
    for m in (hiseg.BinaryMaskBilateralFilter(), hiseg.MorphologicalBilateralFilter(), hiseg.FastBilateralFilter(),
              hiseg.BilateralFilter(kernel_size=3)):
        m = m.to(DEV)
        s = _input("soft_odd").reshape(1, 3, 37, 53)
        keep = s.clone()
        ws = torch.zeros(1, 3, 37, 106, device=DEV)
        ws[..., ::2] = s
        assert torch.equal(m(ws[..., ::2]), m(s)), type(m).__name__
        assert torch.equal(s, keep)


def test_empty_inputs_return_empty_tensors():
    import hiseg
    for m in (hiseg.BinaryMaskEdgeSmoothing(), hiseg.BinaryMaskBilateralFilter(), hiseg.MorphologicalBilateralFilter(),
              hiseg.FastBilateralFilter(), hiseg.BilateralFilter()):
        m = m.to(DEV)
        for shape in ((0, 1, 8, 8), (2, 0, 8, 8)):
            y = m(torch.zeros(shape, device=DEV))
            assert y.shape == shape and y.numel() == 0
    y = hiseg.MultiClassEdgeSmoothing(device=DEV).smooth_predictions(torch.zeros(0, 3, 8, 8, device=DEV))
    assert y.shape == (0, 3, 8, 8)
