"""Boundary refinement stage and active-contour loss: module surface, state_dict parity with the reference's key
names, initial values, refusals (no GPU)."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from helpers import b0_kwargs, hiseg_kwargs


def _head(**kw):
    from hiseg.layers import RefinedHierarchicalSegmentationHead
    args = dict(in_channels=64, mid_channels=64, num_classes=3, mask_size=(32, 24), use_attention_module=True,
                use_contour_detection=True, use_distance_transform=True, normalization_type="batchnorm",
                hierarchical_base_channels=32, hierarchical_depth=3)
    args.update(kw)
    return RefinedHierarchicalSegmentationHead(**args)


def _ref_keys():
    with open(os.path.join(GOLDEN, "state_keys_refine.json")) as f:
        return json.load(f)


def test_head_and_loss_construct_with_the_flags():
    import hiseg
    head = _head(use_boundary_refinement=True)
    assert head.use_boundary_refinement is True
    assert isinstance(head.boundary_refiner, hiseg.BoundaryRefinementModule)
    assert _head().use_boundary_refinement is False and not hasattr(_head(), "boundary_refiner")
    loss = hiseg.RefinedHierarchicalLoss(use_active_contour_loss=True, active_contour_weight=0.25)
    assert loss.use_active_contour_loss is True and loss.active_contour_weight == 0.25
    assert hiseg.RefinedHierarchicalLoss().use_active_contour_loss is False


def test_model_factory_passes_the_flag_through():
    import hiseg
    kw = hiseg_kwargs(dict(b0_kwargs(), use_boundary_refinement=True))
    model = hiseg.create_rgb_hierarchical_model(**kw)
    assert model.segmentation_head.use_boundary_refinement
    assert "segmentation_head.boundary_refiner.blend_weight" in model.state_dict()


def test_state_dict_keys_and_shapes_match_the_reference():
    ref = _ref_keys()
    sd = _head(use_boundary_refinement=True).state_dict()
    mine = {k: list(v.shape) for k, v in sd.items() if k.startswith("boundary_refiner.")}
    assert mine == ref
    assert list(mine) == list(ref)   # same order
    assert {k.split(".")[2] for k in ref if "edge_conv" in k} == {"0", "1", "3", "4", "6"}


def test_reference_named_state_dict_loads_strictly():
    from hiseg.layers import BoundaryRefinementModule
    ref = {k[len("boundary_refiner."):]: torch.full(shape, 0.5) if shape else torch.tensor(0.5)
           for k, shape in _ref_keys().items()}
    ref = {k: (v.long() if k.endswith("num_batches_tracked") else v) for k, v in ref.items()}
    m = BoundaryRefinementModule(3, 32, "batchnorm")
    m.load_state_dict(ref, strict=True)
    assert float(m.blend_weight) == 0.5 and m.blend_weight.dim() == 0


def test_initial_values():
    from hiseg.layers import BoundaryRefinementModule, LayerNorm2d
    torch.manual_seed(3)
    m = BoundaryRefinementModule()   # the reference's defaults: layernorm2d, relu
    assert isinstance(m.edge_conv[1], LayerNorm2d) and isinstance(m.edge_conv[2], torch.nn.ReLU)
    assert m.blend_weight.dim() == 0 and float(m.blend_weight) == pytest.approx(0.01)
    for i in (0, 3, 6):
        c = m.edge_conv[i]
        assert float(c.bias.abs().max()) == 0.0
        fan_in = c.weight[0].numel()
        fan_out = c.weight.shape[0] * c.weight[0, 0].numel()
        bound = 0.1 * (6.0 / (fan_in + fan_out)) ** 0.5   # xavier_uniform_(gain=0.1)
        assert float(c.weight.abs().max()) <= bound
        assert float(c.weight.abs().max()) > 0.8 * bound
    assert [tuple(m.edge_conv[i].weight.shape) for i in (0, 3, 6)] == [(32, 3, 3, 3), (32, 32, 3, 3), (3, 32, 1, 1)]


def test_cpu_tensors_are_refused():
    import hiseg
    from hiseg.layers import BoundaryRefinementModule
    m = BoundaryRefinementModule(3, 32, "batchnorm").eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        m(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        m.train()(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        hiseg.active_contour_term(torch.zeros(1, 3, 4, 4))
    loss = hiseg.RefinedHierarchicalLoss(use_active_contour_loss=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long), {})


@pytest.mark.parametrize("H,W", [(1, 8), (8, 1), (1, 1)])
def test_sizes_below_two_are_a_bad_argument(H, W):
    """Refused by the library before any pointer is looked at (HISEG_ERR_BAD_ARG = -1), in both features."""
    from hiseg import _lib as L
    lib = L.lib()
    assert lib.hiseg_edge_map_fwd(None, 2, H, W, None, None, None, None, 0, 0, None, None) == -1
    assert b"at least 2" in lib.hiseg_last_error_string()
    assert lib.hiseg_boundary_blend_fwd(None, None, 4, None, None, None, 2, H, W, None, None, None) == -1
    assert lib.hiseg_boundary_blend_bwd(None, None, 4, None, None, None, 2, H, W, None, 4, None, None, None) == -1
    assert lib.hiseg_edge_map_bwd(None, None, 0, 0, None, None, None, 2, H, W, None, None, None) == -1
    assert lib.hiseg_boundary_refine_fused(None, 2, H, W, *([None] * 13)) == -1
    assert lib.hiseg_active_contour_fwd(None, 2, H, W, None, None, None) == -1
    assert lib.hiseg_active_contour_bwd(None, 2, H, W, None, None, None, None) == -1
    assert b"at least 2" in lib.hiseg_last_error_string()


def test_workspace_queries():
    from hiseg import _lib as L
    lib = L.lib()
    P = 3 * 9 * 7
    assert lib.hiseg_edge_map_ws(3, 9, 7) > 0
    assert lib.hiseg_boundary_bwd_ws(3, 9, 7) >= 7 * P     # dE + six difference gradients per pixel
    assert lib.hiseg_active_contour_ws(3, 9, 7) >= P       # the class-1 probability


def test_traced_export_refuses_a_boundary_refiner():
    import hiseg
    from hiseg import export
    kw = hiseg_kwargs(dict(b0_kwargs(), use_boundary_refinement=True))
    model = hiseg.create_rgb_hierarchical_model(**kw).eval()
    with pytest.raises(NotImplementedError, match="boundary refiner"):
        export._head_spec(model, "none")
    from hiseg import onnx_graph
    with pytest.raises(NotImplementedError, match="boundary refiner"):
        onnx_graph.emit_rgb_head(None, model, {}, None, None, None, (96, 128), ["logits"])
    plain = hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs())).eval()
    export.refuse_boundary_refiner(plain)   # no refiner: nothing to refuse


@pytest.mark.parametrize("flag", ["use_progressive_upsampling", "use_subpixel_conv"])
def test_other_decoders_still_raise(flag):
    with pytest.raises(NotImplementedError, match="progressive upsampling / sub-pixel"):
        _head(**{flag: True})
