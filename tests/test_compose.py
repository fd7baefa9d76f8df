"""Full-frame instance composition, the parts that need no GPU: the C ABI's symbols and argument checks, the colour
table against the reference's (tests/golden/compose.npz, gen_compose_golden.py) and the serving hook's surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

import filler
from conftest import ROOT
from helpers import b0_kwargs, hiseg_kwargs, load
from test_abi import header_functions

ENTRY_POINTS = ("hiseg_compose_words_per_row", "hiseg_roi_mask_classify_fwd", "hiseg_roi_mask_pack_fwd",
                "hiseg_instance_map_fwd", "hiseg_instance_overlay_fwd")
BAD_ARG = -1


def test_symbols_are_declared_exported_and_bound():
    from hiseg import _lib as L
    lib = L.lib()
    declared = header_functions(["hiseg_compose.h"])
    assert sorted(ENTRY_POINTS) == declared
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in L.EXPORTED, name
    mk = open(os.path.join(ROOT, "human-instance-segmentation_amd", "Makefile")).read()
    assert "csrc/compose.hip" in mk and "hiseg_compose.h" in mk
    assert [lib.hiseg_compose_words_per_row(w) for w in (-3, 0, 1, 32, 33, 96)] == [0, 0, 1, 1, 2, 3]


def test_invalid_arguments_are_refused_before_any_launch():
    from hiseg import _lib as L
    lib = L.lib()

    def err():
        return lib.hiseg_last_error_string()

    fake = 1 << 20      # never dereferenced: every call below is refused, or is empty and launches nothing
    classify, pack = lib.hiseg_roi_mask_classify_fwd, lib.hiseg_roi_mask_pack_fwd
    compose, overlay = lib.hiseg_instance_map_fwd, lib.hiseg_instance_overlay_fwd
    for mh, mw in ((0, 8), (8, 0), (0, 0)):
        assert classify(fake, 2, mh, mw, 0.5, fake, fake, fake, None) == BAD_ARG
        assert b"mh*mw == 0" in err()
        assert pack(fake, 2, mh, mw, fake, fake, fake, None) == BAD_ARG
        assert b"mh*mw == 0" in err()
        assert compose(fake, fake, fake, 2, mh, mw, 1, 8, 8, fake, None) == BAD_ARG
        assert b"mh*mw == 0" in err()
    assert classify(fake, -1, 4, 4, 0.5, fake, fake, fake, None) == BAD_ARG and b"negative N" in err()
    assert pack(fake, -1, 4, 4, fake, fake, fake, None) == BAD_ARG and b"negative N" in err()
    assert compose(fake, fake, fake, -1, 4, 4, 1, 8, 8, fake, None) == BAD_ARG and b"negative N" in err()
    assert overlay(fake, fake, fake, -1, 1, 8, 8, 0.5, fake + 64, None) == BAD_ARG and b"negative N" in err()
    assert compose(fake, fake, fake, 1, 4, 4, 1, -8, 8, fake, None) == BAD_ARG and b"negative frame" in err()
    for hole in range(4):
        a = [fake, fake, fake, fake]
        a[hole] = None
        assert classify(a[0], 2, 4, 4, 0.5, a[1], a[2], a[3], None) == BAD_ARG and b"null" in err(), hole
        assert pack(a[0], 2, 4, 4, a[1], a[2], a[3], None) == BAD_ARG and b"null" in err(), hole
        assert compose(a[0], a[1], a[2], 2, 4, 4, 1, 8, 8, a[3], None) == BAD_ARG and b"null" in err(), hole
        assert overlay(a[0], a[1], a[2], 2, 1, 8, 8, 0.5, a[3], None) == BAD_ARG and b"null" in err(), hole
    assert overlay(fake, fake, fake, 2, 1, 8, 8, 0.5, fake, None) == BAD_ARG and b"alias" in err()
    assert overlay(fake + 4, fake, fake, 2, 1, 8, 8, 0.5, fake + 64, None) == BAD_ARG and b"aligned" in err()
    # empty problems are fine, launch nothing and need no addresses
    assert classify(None, 0, 4, 4, 0.5, None, None, None, None) == 0
    assert pack(None, 0, 4, 4, None, None, None, None) == 0
    assert compose(None, None, None, 0, 4, 4, 0, 8, 8, None, None) == 0
    assert compose(None, None, None, 3, 4, 4, 2, 0, 8, None, None) == 0
    assert overlay(None, None, None, 0, 2, 8, 0, 0.5, None, None) == 0


def test_cpu_tensors_raise():
    import hiseg
    from hiseg import ops
    logits, masks = torch.zeros(2, 3, 4, 4), torch.zeros(2, 1, 4, 4)
    rois = torch.tensor([[0, 0, 0, 1, 1.0]] * 2)
    bits, score = torch.zeros(2, 4, 1, dtype=torch.int32), torch.ones(2)
    label = torch.zeros(1, 8, 8, dtype=torch.int32)
    image, colors = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.uint8)
    for call in (lambda: ops.roi_mask_classify(logits), lambda: ops.roi_mask_pack(masks),
                 lambda: ops.compose_instance_map(bits, score, rois, (1, 8, 8), 4),
                 lambda: ops.instance_overlay(label, image, colors, 0.5),
                 lambda: hiseg.InstanceMapComposer()(logits, rois, (1, 8, 8)),
                 lambda: hiseg.InstanceMapComposer(from_logits=False)(masks, rois, (1, 8, 8)),
                 lambda: hiseg.InstanceMapComposer().overlay(label, image, colors)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


@pytest.mark.parametrize("n", (1, 2, 9, 70))
def test_instance_colors_are_the_reference_s(n):
    import hiseg
    c = hiseg.instance_colors(n)
    assert c.dtype == torch.uint8 and tuple(c.shape) == (n, 3)
    assert np.array_equal(c.numpy(), load("compose")[f"colors_{n}"])
    assert "import matplotlib" not in open(hiseg.compose.__file__).read()


def test_instance_colors_edge_cases():
    import hiseg
    assert tuple(hiseg.instance_colors(0).shape) == (0, 3)
    with pytest.raises(ValueError):
        hiseg.instance_colors(-1)


def test_composer_resolves_the_frame_size():
    import hiseg
    c = hiseg.InstanceMapComposer()
    assert c.score_threshold == 0.5 and c.from_logits and c.frame_size is None
    assert c.resolve_frame_size((2, 5, 7)) == (2, 5, 7)
    with pytest.raises(ValueError, match="frame size"):
        c.resolve_frame_size()
    with pytest.raises(ValueError, match="frame size"):
        c.resolve_frame_size((5, 7))          # no batch size anywhere
    c = hiseg.InstanceMapComposer(frame_size=(480, 640), score_threshold=0.25, from_logits=False)
    assert c.resolve_frame_size((3,)) == (3, 480, 640) and c.resolve_frame_size((2, 5, 7)) == (2, 5, 7)
    c = hiseg.InstanceMapComposer(frame_size=(4, 480, 640))
    assert c.resolve_frame_size() == (4, 480, 640) and c.resolve_frame_size((9, 11)) == (4, 9, 11)
    with pytest.raises(ValueError):
        hiseg.InstanceMapComposer(frame_size=(1, 2, 3, 4))
    assert not list(c.state_dict())


def _model():
    import hiseg
    torch.manual_seed(0)
    return filler.fill_module(hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))).eval()


def test_wrapper_without_a_composer_keeps_its_signature():
    import inspect
    import hiseg
    model = _model()
    w = hiseg.RGBHierarchicalExportWrapper(model)
    assert w.compose is None and w.binary_post is None and w.instance_post is None
    params = list(inspect.signature(hiseg.RGBHierarchicalExportWrapper.__init__).parameters)
    assert params == ["self", "model", "image_size", "dilation_pixels", "binary_post", "instance_post", "compose"]
    assert list(inspect.signature(w.forward).parameters) == ["images", "rois"]
    c = hiseg.InstanceMapComposer(from_logits=False)
    w = hiseg.RGBHierarchicalExportWrapper(model, compose=c)
    assert w.compose is c and not any(k.startswith("compose") for k in w.state_dict())
    # the traced contract of a wrapper without a composer still has two outputs
    images = torch.from_numpy(filler.uniform(41, (1, 3, 96, 128)))
    rois = torch.from_numpy(filler.box_rois(42, 1, 2))
    ep = torch.export.export(hiseg.RGBHierarchicalExportWrapper(model).eval(), (images, rois))
    assert len(ep.graph_signature.user_outputs) == 2


def test_traced_export_refuses_a_wrapper_with_a_composer():
    import hiseg
    wrapper = hiseg.RGBHierarchicalExportWrapper(_model(), compose=hiseg.InstanceMapComposer(from_logits=False)).eval()
    images = torch.from_numpy(filler.uniform(41, (2, 3, 96, 128)))
    rois = torch.from_numpy(filler.box_rois(42, 2, 2))
    with pytest.raises(Exception) as info:
        torch.export.export(wrapper, (images, rois))
    chain, e = [], info.value
    while e is not None:
        chain.append(e)
        e = e.__cause__ or e.__context__
    assert any(isinstance(c, NotImplementedError) or "NotImplementedError" in str(c) for c in chain), chain
    assert any("compose is set" in str(c) for c in chain), chain
