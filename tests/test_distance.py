"""Distance-aware loss without a GPU: the numpy restatement (tests/distance_oracle.py) against the reference's
recorded results (tests/golden/distance.npz, gen_distance_golden.py), and the Python surface of hiseg.distance_loss.

d2 and the weight map are compared bit for bit (the weight is a function of an exact integer and a double table);
the loss scalars to 1e-6 (the restatement sums in float64, the reference in float32 over at most 2880 pixels)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import distance_oracle as O
from conftest import GOLDEN
from helpers import load

MAP_CASES = ["m1x1", "m1x7", "m7x1", "m2x3", "m9x7", "m40x36", "m56x56", "m64x48", "all0", "all1", "all2", "m02",
             "pyth", "mixed"]
S_VARIANTS = ["plain", "cw", "focal2", "focal15", "adaptive", "inst_zeros", "inst_straddle", "inst_missing",
              "adaptive_plain", "nob", "tied"]
B_VARIANTS = ["plain", "cw", "focal2", "focal15", "adaptive"]
LOSS_CASES = [("s", v) for v in S_VARIANTS] + [("b", v) for v in B_VARIANTS]


@pytest.fixture(scope="module")
def G():
    return load("distance")


@pytest.fixture(scope="module")
def surface():
    with open(os.path.join(GOLDEN, "distance_surface.json")) as f:
        return json.load(f)


def variant_setup(G, tag, name):
    """(constructor kwargs, adaptive (boundary, instance) or None, inst [N,H,W] or None, present [N] or None,
    logits) of a recorded loss case -- the table of gen_distance_golden.variants, restated as data."""
    cw = torch.from_numpy(G["factory_class_weights"])
    strad = G[f"{tag}_straddle"]
    n = strad.shape[0]
    table = {
        "plain": ({}, None, None), "cw": ({"class_weights": cw}, None, None),
        "focal2": ({"class_weights": cw, "use_focal": True, "focal_gamma": 2.0}, None, None),
        "focal15": ({"use_focal": True, "focal_gamma": 1.5, "ce_weight": 0.7, "dice_weight": 1.3}, None, None),
        "adaptive": ({"class_weights": cw}, (6.5, 0.5), "straddle"),
        "inst_zeros": ({}, None, "zeros"), "inst_straddle": ({"boundary_width": 3}, None, "straddle"),
        "inst_missing": ({"class_weights": cw}, None, "missing"),
        "adaptive_plain": ({"boundary_width": 8}, (2.25, 3.0), None),
        "nob": ({"boundary_width": 1, "boundary_weight": 1.2}, None, None),
        "tied": ({"boundary_width": 5, "boundary_weight": 3.0}, None, None),
    }
    kw, adaptive, inst_kind = table[name]
    inst = present = None
    if inst_kind == "zeros":
        inst, present = np.zeros_like(strad), np.ones(n, bool)
    elif inst_kind == "straddle":
        inst, present = strad, np.ones(n, bool)
    elif inst_kind == "missing":
        inst, present = strad.copy(), np.ones(n, bool)
        present[1] = False
    x = G[f"{tag}_{name}_x"] if f"{tag}_{name}_x" in G.files else G[f"{tag}_x"]
    return dict(kw), adaptive, inst, present, x


def effective_weights(kw, adaptive):
    bw, isw = kw.get("boundary_weight", 2.0), kw.get("instance_sep_weight", 3.0)
    if adaptive is not None:   # clamp(parameter, 1, 5) of the f32 parameters
        bw, isw = (float(np.clip(np.float32(v), np.float32(1.0), np.float32(5.0))) for v in adaptive)
    return bw, isw


@pytest.mark.parametrize("case", MAP_CASES)
def test_restatement_weight_maps_equal_fixture(G, case):
    t = G[f"{case}_t"].astype(np.int64)
    for width in G["widths"]:
        width = int(width)
        for pi, (bw, isw) in enumerate(G["pairs"]):
            w, d2 = O.weight_map(t, width, float(bw), float(isw))
            assert np.array_equal(d2, G[f"{case}_d2_w{width}"].astype(np.int32)), (case, width)
            assert np.array_equal(w, G[f"{case}_w_w{width}_p{pi}"]), (case, width, pi)


def test_restatement_no_site_masks_use_the_virtual_site(G):
    """{0}, {2} and {0,2} masks have no site: the recorded distances are those to one site at row -1, column 0."""
    yy, xx = np.mgrid[0:8, 0:8]
    want = np.minimum((yy + 1) ** 2 + xx ** 2, 64)
    for case in ("all0", "all2", "m02"):
        assert np.array_equal(G[f"{case}_d2_w8"][0], want), case
    assert np.array_equal(G["all1_d2_w8"][0], np.zeros((8, 8)))
    assert np.allclose(G["all0_w_w5_p0"][0, 0, :3], [1.8, 1.717, 1.553], atol=1e-3)
    assert np.allclose(G["all0_w_w5_p0"][0, 1, :2], [1.6, 1.553], atol=1e-3)


def test_restatement_unclipped_distance_equals_fixture(G):
    for case in ("m9x7", "m40x36"):
        d = O.boundary_distance(G[f"{case}_t"][0].astype(np.int64), 64.0)
        assert np.array_equal(d, G[f"{case}_dist64"]), case


@pytest.mark.parametrize("tag,name", LOSS_CASES)
def test_restatement_loss_equals_fixture(G, tag, name):
    kw, adaptive, inst, present, x = variant_setup(G, tag, name)
    t = G[f"{tag}_t"].astype(np.int64)
    bw, isw = effective_weights(kw, adaptive)
    w, d2 = O.weight_map(t, kw.get("boundary_width", 5), bw, isw, inst, present)
    assert np.array_equal(d2, G[f"{tag}_{name}_d2"].astype(np.int32))
    assert np.array_equal(w, G[f"{tag}_{name}_w"])
    cw = kw.get("class_weights")
    vals, grad = O.loss(x, t, w, None if cw is None else cw.numpy(), kw.get("use_focal", False),
                        kw.get("focal_gamma", 2.0), kw.get("ce_weight", 1.0), kw.get("dice_weight", 1.0))
    ref = G[f"{tag}_{name}_vals"]
    for i, k in enumerate(G["dict_keys"]):
        assert vals[str(k)] == pytest.approx(ref[i], rel=1e-6, abs=1e-6), k
    if adaptive is not None:   # the dict reports the unclamped parameters
        assert tuple(ref[5:]) == tuple(float(np.float32(v)) for v in adaptive)
    rg = G[f"{tag}_{name}_grad"]
    assert np.abs(grad - rg).max() <= 1e-5 * np.abs(rg).max()
    if name == "nob":
        assert ref[3] == 0.0 and w.max() <= 1.5


def test_factory_class_weights_equal_fixture(G):
    import hiseg
    ratios = dict(zip(("background", "target", "non_target"), (float(v) for v in G["pixel_ratios"])))
    loss = hiseg.create_distance_aware_loss(ratios)
    assert isinstance(loss, hiseg.DistanceAwareSegmentationLoss)
    assert np.array_equal(loss.class_weights.numpy(), G["factory_class_weights"])
    assert np.allclose(O.class_weights_from_ratios(ratios), G["factory_class_weights"], rtol=1e-6)
    given = hiseg.create_distance_aware_loss(ratios, separation_aware_weights={"background": 0.5, "target": 1.5,
                                                                               "non_target": 1.0})
    assert given.class_weights.tolist() == [0.5, 1.5, 1.0]


def test_surface_matches_the_recorded_names(surface):
    import hiseg
    from hiseg.distance_loss import LazyDistanceLossDict
    names = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert names(hiseg.DistanceAwareSegmentationLoss) == surface["ctor_DistanceAwareSegmentationLoss"]
    assert names(hiseg.AdaptiveBoundaryLoss) == surface["ctor_AdaptiveBoundaryLoss"]
    assert names(hiseg.create_distance_aware_loss) == surface["factory_args"]
    assert names(hiseg.DistanceAwareSegmentationLoss.forward) == surface["forward_args"]
    assert names(hiseg.AdaptiveBoundaryLoss.forward) == surface["forward_args"]
    ad = hiseg.create_distance_aware_loss({"background": 0.5, "target": 0.3, "non_target": 0.2}, adaptive=True)
    assert isinstance(ad, hiseg.AdaptiveBoundaryLoss)
    assert sorted(ad.state_dict().keys()) == surface["adaptive_state_keys"]
    assert ad.boundary_weight.item() == 2.0 and ad.instance_weight.item() == 3.0
    assert (ad.adaptation_rate, ad.min_weight, ad.max_weight) == (0.01, 1.0, 5.0)
    d = LazyDistanceLossDict(torch.arange(10.0), ("boundary_weight", "instance_weight"))
    assert list(d) == ["total_loss", "ce_loss", "dice_loss", "boundary_accuracy", "avg_boundary_weight",
                       "boundary_weight", "instance_weight"]
    assert d["dice_loss"] == 2.0 and d["boundary_weight"] == 8.0 and d["instance_weight"] == 9.0


def test_cpu_tensors_raise():
    import hiseg
    from hiseg import ops
    x, t = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    loss = hiseg.DistanceAwareSegmentationLoss()
    with pytest.raises(RuntimeError, match="GPU only"):
        loss(x, t)
    with pytest.raises(RuntimeError, match="GPU only"):
        hiseg.AdaptiveBoundaryLoss(loss)(x, t)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.boundary_distance(t[0], 5.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.boundary_weight_map(t, 5, 2.0, 3.0)


def test_argument_validation():
    import hiseg
    loss = hiseg.DistanceAwareSegmentationLoss()
    with pytest.raises(ValueError, match="4D"):
        loss(torch.zeros(3, 4, 4), torch.zeros(4, 4, dtype=torch.int64))
    from hiseg.distance_loss import _instance_maps
    with pytest.raises(ValueError, match="entries"):
        _instance_maps([{}], 2, 4, 4, "cpu")
    with pytest.raises(ValueError, match="instance_distances"):
        _instance_maps([{"instance_distances": torch.zeros(3, 4)}, {}], 2, 4, 4, "cpu")
    inst, present = _instance_maps([{"instance_distances": torch.ones(4, 4)}, {}], 2, 4, 4, "cpu")
    assert present.tolist() == [1, 0] and float(inst[0].min()) == 1.0 and float(inst[1].max()) == 0.0
    assert _instance_maps([{}, None], 2, 4, 4, "cpu") == (None, None)
    assert _instance_maps([], 2, 4, 4, "cpu") == (None, None)


def test_library_argument_checks_without_a_launch():
    """Shape and class-count checks that are made before any tensor reaches the GPU."""
    from hiseg import _lib as L
    lib = L.lib()
    assert lib.hiseg_distance_transform(None, 1, 4, 4, 2, 9, 0, None, None, None) == -1
    assert b"null pointer" in lib.hiseg_last_error_string()
    assert lib.hiseg_distance_loss_fwd(None, None, None, 0, 4, 4, None, 0, 2.0, 1.0, 1.0, None, None, None) == -2
    assert lib.hiseg_distance_resident(128, 96) == 1 and lib.hiseg_distance_resident(256, 256) == 0
    assert lib.hiseg_distance_ws(2, 8, 8) > 0


class _Fake(torch.Tensor):
    """A tensor that claims to live on the GPU, for the checks that come after the device check."""
    @property
    def is_cuda(self):
        return True


def test_class_count_and_target_shape_are_checked():
    import hiseg
    loss = hiseg.DistanceAwareSegmentationLoss()
    x4 = torch.zeros(2, 4, 5, 5).as_subclass(_Fake)
    with pytest.raises(ValueError, match="3 classes"):
        loss(x4, torch.zeros(2, 5, 5, dtype=torch.int64))
    x3 = torch.zeros(2, 3, 5, 5).as_subclass(_Fake)
    with pytest.raises(ValueError, match="targets"):
        loss(x3, torch.zeros(2, 5, 4, dtype=torch.int64))
    bad = hiseg.DistanceAwareSegmentationLoss(class_weights=torch.ones(4))
    with pytest.raises(ValueError, match="3 class weights"):
        bad(x3, torch.zeros(2, 5, 5, dtype=torch.int64))
