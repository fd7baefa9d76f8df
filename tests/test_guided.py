"""The guided filter and the serving post-filter hooks without a GPU: the module surface against the reference's
(buffer values from tests/golden/guided.npz, written by gen_guided_golden.py), argument checking of the C entry
and of the Python layers, and the wrapper's hooks."""
import os

import numpy as np
import pytest
import torch

import filler
from conftest import GOLDEN
from helpers import b0_kwargs, hiseg_kwargs
from test_abi import header_functions

BAD_ARG = -1


def test_header_declares_and_library_binds_the_entry_point():
    from hiseg import _lib as L
    assert "hiseg_guided_filter_fwd" in header_functions(["hiseg_post.h"])
    assert hasattr(L.lib(), "hiseg_guided_filter_fwd") and "hiseg_guided_filter_fwd" in L.EXPORTED


def test_class_surface_and_box_kernel_match_the_reference():
    import hiseg
    gold = np.load(os.path.join(GOLDEN, "guided.npz"))
    m = hiseg.EdgePreservingFilter()
    assert (m.radius, m.eps, m.kernel_size) == (2, 0.01, 5)
    for radius, eps in ((2, 0.01), (4, 1e-3), (8, 1e-4)):
        m = hiseg.EdgePreservingFilter(radius=radius, eps=eps)
        k = 2 * radius + 1
        assert (m.radius, m.eps, m.kernel_size) == (radius, eps, k)
        sd = m.state_dict()
        assert list(sd) == ["box_kernel"] and tuple(sd["box_kernel"].shape) == (1, 1, k, k)
        assert sd["box_kernel"].dtype == torch.float32
        want = gold[f"buf/box_kernel/{radius}"]
        assert want.shape == (1, 1, k, k)
        np.testing.assert_array_equal(sd["box_kernel"].numpy(), want)
        np.testing.assert_array_equal(want, np.full((1, 1, k, k), np.float32(1) / np.float32(k * k)))
    assert "EdgePreservingFilter" in hiseg.postprocess.__all__


def test_reference_named_state_dict_loads_strictly():
    import hiseg
    gold = np.load(os.path.join(GOLDEN, "guided.npz"))
    m = hiseg.EdgePreservingFilter(radius=4, eps=1e-3)
    res = m.load_state_dict({"box_kernel": torch.from_numpy(gold["buf/box_kernel/4"])}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with pytest.raises(RuntimeError):
        m.load_state_dict({"box_kernel": torch.from_numpy(gold["buf/box_kernel/2"])}, strict=True)   # 5x5 into 9x9


def test_cpu_tensors_and_bad_shapes_are_refused():
    import hiseg
    from hiseg import ops
    m = hiseg.EdgePreservingFilter()
    for x, g in ((torch.zeros(1, 1, 8, 8), None), (torch.zeros(1, 8, 8), None),
                 (torch.zeros(1, 1, 8, 8), torch.zeros(1, 3, 8, 8))):
        with pytest.raises(RuntimeError, match="GPU only"):
            m(x, g)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.guided_filter(torch.zeros(1, 1, 8, 8), None, 2, 0.01)
    with pytest.raises(ValueError):
        m(torch.zeros(8, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 8, 8), torch.zeros(1, 8, 8))
    for radius in (0, 17):
        with pytest.raises(ValueError, match="radius"):
            hiseg.EdgePreservingFilter(radius=radius)


def test_bad_arguments_are_refused_without_touching_the_gpu():
    from hiseg import _lib as L
    lib = L.lib()
    f = lib.hiseg_guided_filter_fwd
    err = lib.hiseg_last_error_string
    fake, fake2 = 1 << 20, 1 << 21   # never dereferenced: every call below is refused before a launch
    for radius in (0, 17):
        assert f(None, None, None, 1, 1, 1, 8, 8, radius, 0.01, 0, None) == BAD_ARG
        assert b"radius" in err()
        assert f(fake, None, fake2, 1, 1, 1, 8, 8, radius, 0.01, 0, None) == BAD_ARG
    assert f(None, None, None, 1, 2, 3, 8, 8, 2, 0.01, 0, None) == BAD_ARG
    assert f(fake, fake, fake2, 1, 2, 3, 8, 8, 2, 0.01, 0, None) == BAD_ARG
    assert b"broadcast" in err()
    assert f(fake, fake, fake2, 1, 3, 2, 8, 8, 2, 0.01, 1, None) == BAD_ARG
    assert b"broadcast" in err()
    assert f(None, None, fake2, 1, 1, 1, 8, 8, 2, 0.01, 0, None) == BAD_ARG
    assert b"null" in err()
    assert f(fake, fake, None, 1, 1, 3, 8, 8, 2, 0.01, 0, None) == BAD_ARG
    assert b"null" in err()
    assert f(fake, None, fake, 1, 1, 1, 8, 8, 2, 0.01, 0, None) == BAD_ARG      # x and out are distinct
    assert b"alias" in err()
    assert f(fake, fake2, fake2, 1, 1, 3, 8, 8, 2, 0.01, 0, None) == BAD_ARG
    # empty problems are fine and launch nothing (an empty tensor has no address); a bad radius is still refused
    assert f(None, None, None, 0, 1, 3, 8, 8, 2, 0.01, 0, None) == 0
    assert f(None, None, None, 2, 1, 1, 0, 8, 16, 0.01, 1, None) == 0
    assert f(None, None, None, 2, 0, 0, 8, 8, 1, 0.01, 0, None) == 0
    assert f(None, None, None, 0, 1, 1, 8, 8, 0, 0.01, 0, None) == BAD_ARG


def _model():
    import hiseg
    torch.manual_seed(0)
    return filler.fill_module(hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))).eval()


def test_wrapper_stores_the_hooks():
    import hiseg
    model = _model()
    w = hiseg.RGBHierarchicalExportWrapper(model)
    assert w.binary_post is None and w.instance_post is None
    assert not any(k.startswith(("binary_post", "instance_post")) for k in w.state_dict())
    bp, ip = hiseg.EdgePreservingFilter(radius=4), hiseg.BinaryMaskEdgeSmoothing()
    w = hiseg.RGBHierarchicalExportWrapper(model, (96, 128), 1, bp, ip)
    assert w.binary_post is bp and w.instance_post is ip and w.image_size == (96, 128) and w.dilation_pixels == 1

    def fn(t):
        return t
    w = hiseg.RGBHierarchicalExportWrapper(model, instance_post=fn)    # any callable of one tensor
    assert w.instance_post is fn and w.binary_post is None


@pytest.mark.parametrize("hook", ("binary_post", "instance_post"))
def test_traced_export_refuses_a_wrapper_with_a_hook(hook):
    import hiseg
    wrapper = hiseg.RGBHierarchicalExportWrapper(_model(), **{hook: hiseg.EdgePreservingFilter()}).eval()
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
