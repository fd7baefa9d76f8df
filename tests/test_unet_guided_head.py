"""UNet-guided direct 3-class head: module surface, state_dict parity with the reference's key names, initial values,
refusals and the C ABI's descriptor layouts (no GPU)."""
import ctypes
import json
import os

import pytest
import torch

from conftest import GOLDEN
from helpers import b0_kwargs, hiseg_kwargs

FLAGS = ("use_boundary_refinement", "use_progressive_upsampling", "use_subpixel_conv", "use_contour_detection",
         "use_distance_transform")


def _ref():
    with open(os.path.join(GOLDEN, "state_keys_unet_guided_head.json")) as f:
        return json.load(f)


def _kwargs(**over):
    kw = hiseg_kwargs(b0_kwargs())
    kw.update({f: False for f in FLAGS})
    kw.update(over)
    return kw


def _head(att=True, **kw):
    import hiseg
    return hiseg.PretrainedUNetGuidedSegmentationHead(256, 256, 3, (4, 6), use_attention_module=att,
                                                      normalization_type="batchnorm", **kw)


def _shapes(m):
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def _outside_unet(shapes):
    """The reference fixture was built with a parameter-free smp stand-in: everything outside the smp.Unet."""
    return {k: v for k, v in shapes.items() if not k.startswith("pretrained_unet.model.model.")}


def test_model_without_refinement_flags_has_the_guided_head_and_no_combiner():
    import hiseg
    model = hiseg.create_rgb_hierarchical_model(**_kwargs())
    assert isinstance(model.segmentation_head, hiseg.PretrainedUNetGuidedSegmentationHead)
    assert not hasattr(model, "feature_combiner")
    assert not any(k.startswith("feature_combiner") for k in model.state_dict())
    assert (model.segmentation_head.mask_height, model.segmentation_head.mask_width) == tuple(model.mask_size)
    # the refined path is what it was
    refined = hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))
    assert isinstance(refined.segmentation_head, hiseg.RefinedHierarchicalSegmentationHead)
    assert hasattr(refined, "feature_combiner")


def test_state_dict_keys_and_shapes_match_the_reference():
    import hiseg
    ref = _ref()
    for att, key in ((True, "head"), (False, "head_noatt")):
        mine = _shapes(_head(att))
        assert mine == ref[key] and list(mine) == list(ref[key])   # same keys, shapes and order
    subs = {".".join(k.split(".")[:2]) for k in ref["head"]}
    assert subs == {"input_adjust.weight", "input_adjust.bias", "feature_processor.0", "feature_processor.1",
                    "feature_processor.4", "feature_processor.6", "final_classifier.0", "final_classifier.1",
                    "final_classifier.3", "attention_module.0", "attention_module.2"}
    model = hiseg.create_rgb_hierarchical_model(**_kwargs())
    mine = _outside_unet(_shapes(model))
    assert mine == ref["model"] and list(mine) == list(ref["model"])


def test_final_classifier_bias_initialisation():
    b = _head().final_classifier[3].bias.detach()
    assert b.tolist() == _ref()["final_bias_init"] == [0.0, 0.0, -0.5]


@pytest.mark.parametrize("norm,act", [("batchnorm", "relu"), ("layernorm2d", "silu"), ("batchnorm", "swish"),
                                      ("layernorm2d", "gelu")])
def test_supported_normalisations_and_activations(norm, act):
    import hiseg
    h = hiseg.PretrainedUNetGuidedSegmentationHead(256, 256, 3, 56, use_attention_module=True,
                                                   normalization_type=norm, activation_function=act)
    assert list(_shapes(h)) == [k for k in _ref()["head"] if norm == "batchnorm" or "running_" not in k
                                and "num_batches_tracked" not in k]
    assert (h.mask_height, h.mask_width) == (56, 56)


def test_other_normalisations_raise_as_before():
    import hiseg
    for norm in ("groupnorm", "instancenorm", "mixed_bn_gn"):
        with pytest.raises(NotImplementedError, match="outside the hiseg hot path"):
            hiseg.PretrainedUNetGuidedSegmentationHead(256, normalization_type=norm)
    with pytest.raises(ValueError):
        hiseg.PretrainedUNetGuidedSegmentationHead(256, normalization_type="batchnorm", activation_function="mish")


def test_reference_named_state_dict_round_trips_strictly():
    import hiseg
    ref = _ref()
    model = hiseg.create_rgb_hierarchical_model(**_kwargs())
    sd = {k: (torch.full(shape, 3, dtype=torch.long) if k.endswith("num_batches_tracked")
              else torch.full(shape, 0.25)) for k, shape in ref["model"].items()}
    unet = {k: v for k, v in model.state_dict().items() if k.startswith("pretrained_unet.model.model.")}
    model.load_state_dict({**sd, **unet}, strict=True)
    back = model.state_dict()
    assert list(_outside_unet(back)) == list(ref["model"])
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    head = _head()
    head.load_state_dict({k[len("segmentation_head."):]: v for k, v in sd.items()
                          if k.startswith("segmentation_head.")}, strict=True)


def test_checkpoint_module_loads_a_reference_format_checkpoint(tmp_path):
    import filler
    import hiseg
    src = filler.fill_module(hiseg.create_rgb_hierarchical_model(**_kwargs()))
    path = os.path.join(tmp_path, "guided.pth")
    torch.save({"model_state_dict": src.state_dict(), "epoch": 3, "best_miou": 0.5}, path)
    dst = hiseg.create_rgb_hierarchical_model(**_kwargs())
    hiseg.load_teacher_checkpoint(path, dst)
    a, b = src.state_dict(), dst.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_train_mode_raises():
    import hiseg
    head = _head().train()
    with pytest.raises(NotImplementedError, match="inference only"):
        head(torch.zeros(1, 256, 2, 3), torch.zeros(1, 2, 2, 3))
    model = hiseg.create_rgb_hierarchical_model(**_kwargs()).train()
    with pytest.raises(NotImplementedError, match="inference only"):
        model(torch.zeros(1, 3, 32, 32), torch.tensor([[0, .1, .1, .9, .9]]))


def test_traced_export_raises():
    import hiseg
    model = hiseg.create_rgb_hierarchical_model(**_kwargs()).eval()
    images, rois = torch.zeros(1, 3, 32, 32), torch.tensor([[0, .1, .1, .9, .9]])
    with pytest.raises(NotImplementedError, match="PretrainedUNetGuidedSegmentationHead"):
        torch.jit.trace(model, (images, rois), strict=False)
    with pytest.raises(NotImplementedError, match="PretrainedUNetGuidedSegmentationHead"):
        torch.jit.trace(hiseg.RGBHierarchicalExportWrapper(model), (images, rois), strict=False)
    from hiseg import export
    with pytest.raises(NotImplementedError, match="PretrainedUNetGuidedSegmentationHead"):
        export._head_spec(model, "none")


def test_abi_struct_sizes_and_declared_entry_points():
    from hiseg import _lib as L
    from test_abi import header_functions
    declared = header_functions(["hiseg_guided_head.h"])
    assert set(declared) == {"hiseg_guided_struct_sizes", "hiseg_guided_prep_fwd", "hiseg_guided_attn_fwd",
                             "hiseg_guided_finish_rows", "hiseg_guided_finish_fwd"}
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name) and name in L.EXPORTED, name
    classes = [L.GuidedPrepDesc, L.GuidedAttnDesc, L.GuidedFinishDesc]
    out = (ctypes.c_longlong * len(classes))()
    assert lib.hiseg_guided_struct_sizes(out, len(classes)) == len(classes)
    for cls, size in zip(classes, out):
        assert ctypes.sizeof(cls) == size, (cls.__name__, ctypes.sizeof(cls), size)


def test_bad_descriptors_are_refused_before_any_launch():
    from hiseg import _lib as L
    lib = L.lib()
    d = L.GuidedFinishDesc()
    assert lib.hiseg_guided_finish_fwd(ctypes.byref(d), None) == -1   # HISEG_ERR_BAD_ARG
    a = L.GuidedAttnDesc()
    assert lib.hiseg_guided_attn_fwd(ctypes.byref(a), None) == -1
    p = L.GuidedPrepDesc()
    assert lib.hiseg_guided_prep_fwd(ctypes.byref(p), None) == -1
    # output rows per workgroup: 8 source rows' worth, fewer where the LDS tile would not fit, 0 where one row does not
    assert lib.hiseg_guided_finish_rows(64, 48, 128, 96) == 16
    assert lib.hiseg_guided_finish_rows(8, 12, 8, 12) == 8
    assert lib.hiseg_guided_finish_rows(2, 3, 4, 6) == 4
    assert lib.hiseg_guided_finish_rows(64, 1024, 64, 1024) == 4
    assert lib.hiseg_guided_finish_rows(4096, 4096, 2, 2) == 0
