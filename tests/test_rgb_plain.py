"""Plain RGB model (HierarchicalRGBSegmentationModel): module surface, state_dict parity with the reference's key names
(tests/golden/state_keys_rgb_plain.json), the factory's branches, refusals and the new entry point's declaration
(no GPU)."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

NORMS = {"ln": "layernorm2d", "bn": "batchnorm"}


def _ref():
    with open(os.path.join(GOLDEN, "state_keys_rgb_plain.json")) as f:
        return json.load(f)


def _shapes(m):
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def _same(mine, ref):
    return mine == ref and list(mine) == list(ref)   # same keys, shapes and order


def _model(tag="ln", mask=(11, 20), **kw):
    import hiseg
    return hiseg.create_rgb_hierarchical_model(roi_size=(8, 12), mask_size=mask, normalization_type=NORMS[tag],
                                               use_attention_module=True, **kw)


@pytest.mark.parametrize("tag", ["ln", "bn"])
def test_state_dict_keys_and_shapes_match_the_reference(tag):
    import hiseg
    ref = _ref()
    ext = hiseg.RGBFeatureExtractor(normalization_type=NORMS[tag])
    assert _same(_shapes(ext), ref[f"extractor_{tag}"])
    # 3 -> 64 -> 128 -> 192 -> 256, a residual block after layers 1..3 only
    convs = [m for m in ext.features if isinstance(m, torch.nn.Conv2d)]
    assert [(c.in_channels, c.out_channels) for c in convs] == [(3, 64), (64, 128), (128, 192), (192, 256)]
    assert [i for i, m in enumerate(ext.features) if isinstance(m, hiseg.ResidualBlock)] == [6, 10, 14]
    assert _same(_shapes(_model(tag)), ref[f"model_{tag}"])


def test_extractor_block_quirks():
    """For batchnorm the block takes the given norm and activation; for layernorm2d it is the UNet module's
    ResidualBlock(out_ch) with its defaults, whatever the activation."""
    import hiseg
    bn = hiseg.RGBFeatureExtractor(normalization_type="batchnorm", activation_function="silu")
    assert isinstance(bn.features[6].norm1, torch.nn.BatchNorm2d) and isinstance(bn.features[6].activation, torch.nn.SiLU)
    ln = hiseg.RGBFeatureExtractor(normalization_type="layernorm2d", activation_function="silu")
    assert isinstance(ln.features[2], torch.nn.SiLU)
    assert isinstance(ln.features[6].norm1, hiseg.LayerNorm2d) and isinstance(ln.features[6].activation, torch.nn.ReLU)
    with pytest.raises(NotImplementedError, match="outside the hiseg hot path"):
        hiseg.RGBFeatureExtractor(normalization_type="groupnorm")


@pytest.mark.parametrize("att", [True, False])
def test_plain_head_keys_match_the_reference(att):
    import hiseg
    ref = _ref()["head_att" if att else "head_noatt"]
    head = hiseg.HierarchicalSegmentationHeadUNetV2(256, 256, 3, 56, use_attention_module=att)
    assert _same(_shapes(head), ref)
    # the submodule names of the extended head, always LayerNorm2d + ReLU
    ext = hiseg.ExtendedHierarchicalSegmentationHeadUNetV2(256, 256, 3, 56, use_attention_module=att)
    assert list(_shapes(head)) == list(_shapes(ext))
    assert isinstance(head.shared_features[1], hiseg.LayerNorm2d) and isinstance(head.shared_features[2], torch.nn.ReLU)
    assert (head.mask_height, head.mask_width) == (56, 56)


def test_factory_branches():
    import hiseg
    plain = hiseg.create_rgb_hierarchical_model()   # the factory's default branch
    assert type(plain) is hiseg.HierarchicalRGBSegmentationModel
    assert type(plain.segmentation_head) is hiseg.HierarchicalSegmentationHeadUNetV2
    assert (plain.roi_height, plain.roi_width, plain.mask_height, plain.mask_width) == (28, 28, 56, 56)
    assert not hasattr(plain, "pretrained_unet") and not hasattr(plain, "feature_combiner")
    ra = plain.roi_align
    assert (ra.aligned, ra.spatial_scale, ra.spatial_scale_h, ra.spatial_scale_w) == (False, 640.0, 640.0, 640.0)
    # the activation is not forwarded (rgb.py:354-361, :1014-1027): the default, ReLU
    m = hiseg.create_rgb_hierarchical_model(activation_function="silu", normalization_type="batchnorm")
    assert isinstance(m.rgb_extractor.features[2], torch.nn.ReLU)
    refined = _model("bn", use_contour_detection=True)
    assert type(refined.segmentation_head) is hiseg.RefinedHierarchicalSegmentationHead
    assert _same(_shapes(refined), _ref()["model_refined_bn"])
    with pytest.raises(NotImplementedError, match="multi-scale"):
        hiseg.create_rgb_hierarchical_model(multi_scale=True)
    with pytest.raises(NotImplementedError, match="ROI-UNet"):
        hiseg.create_rgb_hierarchical_model(use_pretrained_unet=True)
    # refusals that stay
    with pytest.raises(NotImplementedError, match="progressive upsampling / sub-pixel"):
        _model(use_progressive_upsampling=True)
    with pytest.raises(NotImplementedError, match="outside the hiseg hot path"):
        hiseg.create_rgb_hierarchical_model(normalization_type="groupnorm")


@pytest.mark.parametrize("tag", ["ln", "bn"])
def test_reference_named_state_dict_round_trips_strictly(tag, tmp_path):
    import filler
    import hiseg
    ref = _ref()[f"model_{tag}"]
    model = _model(tag)
    sd = {k: (torch.full(shape, 3, dtype=torch.long) if k.endswith("num_batches_tracked")
              else torch.full(shape, 0.25)) for k, shape in ref.items()}
    model.load_state_dict(sd, strict=True)
    back = model.state_dict()
    assert list(back) == list(ref) and all(torch.equal(back[k], sd[k]) for k in sd)
    # a reference-format checkpoint through the checkpoint module
    src = filler.fill_module(_model(tag))
    path = os.path.join(tmp_path, "plain.pth")
    torch.save({"model_state_dict": src.state_dict(), "epoch": 3, "best_miou": 0.5}, path)
    dst = _model(tag)
    hiseg.load_teacher_checkpoint(path, dst)
    a, b = src.state_dict(), dst.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_train_mode_raises():
    import hiseg
    images, rois = torch.zeros(1, 3, 32, 32), torch.tensor([[0, .1, .1, .9, .9]])
    model = _model().train()
    with pytest.raises(NotImplementedError, match="inference only"):
        model(images, rois)
    with pytest.raises(NotImplementedError, match="inference only"):
        model.infer(images, rois)
    head = hiseg.HierarchicalSegmentationHeadUNetV2(256, 256, 3, (11, 20)).train()
    with pytest.raises(NotImplementedError, match="inference only"):
        head(torch.zeros(1, 256, 8, 12))


def test_cpu_tensors_raise():
    import hiseg
    images, rois = torch.zeros(1, 3, 32, 32), torch.tensor([[0, .1, .1, .9, .9]])
    model = _model().eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        model(images, rois)
    with pytest.raises(RuntimeError, match="GPU only"):
        model.infer(images, rois)
    with pytest.raises(RuntimeError, match="GPU only"):
        model.segmentation_head(torch.zeros(1, 256, 8, 12))
    with pytest.raises(RuntimeError, match="GPU only"):
        model.rgb_extractor(torch.zeros(1, 3, 8, 12))
    assert hiseg.set_compute_dtype(model, torch.bfloat16).hiseg_dtype == torch.bfloat16


def test_export_wrappers_and_traced_export_raise():
    import hiseg
    model = _model().eval()
    with pytest.raises(NotImplementedError, match="has no UNet"):
        hiseg.RGBHierarchicalExportWrapper(model)
    with pytest.raises(NotImplementedError, match="has no UNet"):
        hiseg.StreamPipelinedExport(model)
    images, rois = torch.zeros(1, 3, 32, 32), torch.tensor([[0, .1, .1, .9, .9]])
    with pytest.raises(NotImplementedError, match="export of the plain"):
        torch.jit.trace(model, (images, rois), strict=False)


def test_entry_point_is_declared_and_bound():
    import ctypes
    from hiseg import _lib as L
    from test_abi import header_functions
    assert "hiseg_hier_combine_resize" in header_functions(["hiseg.h"])
    lib = L.lib()
    assert hasattr(lib, "hiseg_hier_combine_resize") and "hiseg_hier_combine_resize" in L.EXPORTED
    # out-of-range arguments are refused before any launch
    fake = ctypes.c_void_p(1 << 20)
    args = lambda h, w, mh, mw, low=fake: (low, 1, h, w, fake, fake, fake, fake, 1, 1.0, 0, fake, fake, mh, mw,  # noqa: E731
                                            fake, None, None, None)
    assert lib.hiseg_hier_combine_resize(*args(4, 4, 8, 8, low=None)) == -1    # HISEG_ERR_BAD_ARG
    assert b"null pointer" in lib.hiseg_last_error_string()
    assert lib.hiseg_hier_combine_resize(*args(4, 4, 0, 8)) == -2              # HISEG_ERR_BAD_SHAPE
    assert lib.hiseg_hier_combine_resize(*args(0, 4, 8, 8)) == -2
    assert lib.hiseg_hier_combine_resize(*args(64, 64, 16, 16)) == -2          # source window past the LDS
    assert b"source window" in lib.hiseg_last_error_string()
