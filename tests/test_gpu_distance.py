"""Distance transform, boundary weight map and distance-aware loss on the GPU against the reference's recorded
results (tests/golden/distance.npz, gen_distance_golden.py) and the numpy restatement (tests/distance_oracle.py).

Bars.  d2 and the weight map: bit equality (the weight is a function of an exact integer and a host-built double
table).  Loss scalars 1e-5 relative, gradients 1e-5 of the gradient's largest magnitude (the project's bars for
loss values and gradients, tests/test_gpu_train.py); boundary_accuracy 1e-6.  Raw C-ABI calls start from outputs
filled with NaN (-7 for the integer d2), so a launch that covers too little fails."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import distance_oracle as O
import filler
from helpers import b0_kwargs, hiseg_kwargs, load
from test_distance import LOSS_CASES, MAP_CASES, effective_weights, variant_setup

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def G():
    return load("distance")


def dev(a, dtype=None):
    t = torch.as_tensor(np.asarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def raw_weight_map(t, width, bw, isw, inst=None, present=None, dev_w=None, tiled=False):
    """hiseg_distance_weight_map into prefilled outputs: (weights, d2)."""
    from hiseg import _lib as L
    from hiseg import ops
    lib = L.lib()
    N, H, W = t.shape
    d2 = torch.full((N, H, W), -7, dtype=torch.int32, device=DEV)
    w = torch.full((N, H, W), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.full((int(lib.hiseg_distance_ws(N, H, W)),), float("nan"), dtype=torch.float32, device=DEV)
    table = ops._distance_table(width, torch.device(DEV))
    p = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    L.check(lib.hiseg_distance_weight_map(t.data_ptr(), N, H, W, width, table.data_ptr(), float(bw), float(isw),
                                          p(dev_w), p(inst), p(present), int(tiled), d2.data_ptr(), w.data_ptr(),
                                          ws.data_ptr(), L.stream_ptr()), "distance_weight_map")
    return w, d2


def raw_loss(x, t, w, cw, use_focal, gamma, ce_weight, dice_weight, gscale=1.0):
    """hiseg_distance_loss_fwd / _bwd into prefilled outputs: (out[8], dpred)."""
    from hiseg import _lib as L
    lib = L.lib()
    N, _, H, W = x.shape
    ws = torch.full((int(lib.hiseg_distance_ws(N, H, W)),), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    dp = torch.full_like(x, float("nan"))
    g = torch.tensor([gscale], dtype=torch.float32, device=DEV)
    p = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    L.check(lib.hiseg_distance_loss_fwd(x.data_ptr(), t.data_ptr(), w.data_ptr(), N, H, W, p(cw), int(use_focal),
                                        float(gamma), float(ce_weight), float(dice_weight), ws.data_ptr(),
                                        out.data_ptr(), L.stream_ptr()), "distance_loss_fwd")
    L.check(lib.hiseg_distance_loss_bwd(x.data_ptr(), t.data_ptr(), w.data_ptr(), N, H, W, p(cw), int(use_focal),
                                        float(gamma), ws.data_ptr(), g.data_ptr(), dp.data_ptr(), L.stream_ptr()),
            "distance_loss_bwd")
    return out, dp


@pytest.mark.parametrize("case", MAP_CASES)
def test_weight_maps_equal_fixture(G, case):
    t = dev(G[f"{case}_t"], torch.int64)
    for width in (int(v) for v in G["widths"]):
        want_d2 = dev(G[f"{case}_d2_w{width}"], torch.int32)
        for pi, (bw, isw) in enumerate(G["pairs"]):
            want_w = dev(G[f"{case}_w_w{width}_p{pi}"])
            for tiled in (False, True):
                w, d2 = raw_weight_map(t, width, bw, isw, tiled=tiled)
                assert torch.equal(d2, want_d2), (case, width, tiled)
                assert torch.equal(w, want_w), (case, width, pi, tiled)


def test_unclipped_boundary_distance(G):
    from hiseg import ops
    for case in ("m9x7", "m40x36"):
        d = ops.boundary_distance(dev(G[f"{case}_t"][0], torch.int64), 64.0)
        assert d.dtype == torch.float64 and torch.equal(d.cpu(), torch.from_numpy(G[f"{case}_dist64"])), case
    m = blob_masks(np.random.default_rng(41), 3, 33, 29, 5)
    dist, d2 = ops.boundary_distance(dev(m), 1e4, return_d2=True)
    want = np.stack([O.d2_map(x) for x in m])
    assert torch.equal(d2.cpu(), torch.from_numpy(want).to(torch.int32))
    assert torch.equal(dist.cpu(), torch.from_numpy(np.sqrt(want.astype(np.float64))))
    clipped = ops.boundary_distance(dev(m[0]), 4.5)   # a fractional clip on one [H,W] mask
    assert tuple(clipped.shape) == (33, 29)
    assert torch.equal(clipped.cpu(), torch.from_numpy(O.boundary_distance(m[0], 4.5)))


def build_loss(G, tag, name):
    import hiseg
    kw, adaptive, inst, present, x = variant_setup(G, tag, name)
    if "class_weights" in kw:
        kw["class_weights"] = kw["class_weights"].to(DEV)
    loss_fn = hiseg.DistanceAwareSegmentationLoss(**kw)
    if adaptive is not None:
        loss_fn = hiseg.AdaptiveBoundaryLoss(loss_fn).to(DEV)
        with torch.no_grad():
            loss_fn.boundary_weight.fill_(adaptive[0])
            loss_fn.instance_weight.fill_(adaptive[1])
    info = None
    if inst is not None:   # the reference's list of per-sample dicts, CPU tensors, one of them without the key
        info = [{"instance_distances": torch.from_numpy(inst[i])} if present[i] else {} for i in range(len(inst))]
    return loss_fn, kw, adaptive, inst, present, x, info


@pytest.mark.parametrize("tag,name", LOSS_CASES)
def test_loss_matches_fixture(G, tag, name):
    loss_fn, kw, adaptive, inst, present, x, info = build_loss(G, tag, name)
    t = dev(G[f"{tag}_t"], torch.int64)
    pred = dev(x).requires_grad_(True)
    total, d = loss_fn(pred, t, info)
    total.backward()
    base = loss_fn.base_loss if adaptive is not None else loss_fn
    assert torch.equal(base.last["d2"], dev(G[f"{tag}_{name}_d2"], torch.int32))
    assert torch.equal(base.last["weights"], dev(G[f"{tag}_{name}_w"]))
    ref = G[f"{tag}_{name}_vals"]
    keys = [str(k) for k in G["dict_keys"]] + (["boundary_weight", "instance_weight"] if adaptive is not None else [])
    assert list(d.keys()) == keys
    for i, k in enumerate(keys):
        print(f"  {tag}_{name} {k}: {d[k]:.8f} vs {ref[i]:.8f}")
        if k == "boundary_accuracy":
            assert abs(d[k] - ref[i]) <= 1e-6
        else:
            assert d[k] == pytest.approx(ref[i], rel=1e-5), k
    assert float(total.detach()) == pytest.approx(ref[0], rel=1e-5)
    rg = dev(G[f"{tag}_{name}_grad"])
    err = float((pred.grad - rg).abs().max() / rg.abs().max())
    print(f"  {tag}_{name} grad err {err:.2e}")
    assert err <= 1e-5
    # the same through the C ABI into NaN-filled outputs: every output element is written, and identically
    bw, isw = effective_weights(kw, adaptive)
    dev_w = torch.tensor([bw, isw], dtype=torch.float32, device=DEV) if adaptive is not None else None
    w, d2 = raw_weight_map(t, kw.get("boundary_width", 5), bw, isw, None if inst is None else dev(inst),
                           None if inst is None else dev(present, torch.uint8), dev_w)
    assert torch.equal(w, base.last["weights"]) and torch.equal(d2, base.last["d2"])
    out, dp = raw_loss(pred.detach(), t, w, kw.get("class_weights"), kw.get("use_focal", False),
                       kw.get("focal_gamma", 2.0), kw.get("ce_weight", 1.0), kw.get("dice_weight", 1.0))
    assert torch.equal(out[:5], d._out[:5]) and torch.equal(out[5:], torch.zeros(3, device=DEV))
    assert torch.equal(dp, pred.grad)


def test_gpu_instance_maps_and_tensor_form(G):
    """instance_info as GPU tensors in the list, and as one [N,H,W] tensor, equal the CPU-list form."""
    import hiseg
    t, x, strad = dev(G["s_t"], torch.int64), dev(G["s_x"]), G["s_straddle"]
    loss_fn = hiseg.DistanceAwareSegmentationLoss(boundary_width=3)
    want = dev(G["s_inst_straddle_w"])
    for info in ([{"instance_distances": dev(strad[i])} for i in range(3)], dev(strad)):
        total, _ = loss_fn(x, t, info)
        assert torch.equal(loss_fn.last["weights"], want)
        assert float(total.detach()) == pytest.approx(float(G["s_inst_straddle_vals"][0]), rel=1e-5)


def blob_masks(rng, n, h, w, block):
    """Random class masks [n,h,w] of blocks of `block` pixels; sample 1 (if any) has two classes, sample 2 none of
    class 1 (no site)."""
    out = np.zeros((n, h, w), np.int64)
    for i in range(n):
        classes = (0, 1, 2) if i % 3 == 0 else ((0, 1) if i % 3 == 1 else (0, 2))
        low = rng.choice(np.array(classes), size=(-(-h // block), -(-w // block)))
        out[i] = np.kron(low, np.ones((block, block), np.int64))[:h, :w]
    return out


def resident_limit_height(W):
    """The smallest odd H at which an H x W mask no longer takes the LDS-resident kernel."""
    from hiseg import _lib as L
    H = 1
    while L.lib().hiseg_distance_resident(H, W):
        H += 2
    assert L.lib().hiseg_distance_resident(H - 2, W) == 1
    return H


def test_random_sweep_against_restatement():
    from hiseg import _lib as L
    rng = np.random.default_rng(7)
    big_h = resident_limit_height(233)
    sweep = [  # N, H, W, width, tiled variants to run
        (3, 7, 5, 3, (False, True)), (3, 33, 29, 5, (False, True)), (2, 65, 67, 8, (False, True)),
        (2, 129, 71, 20, (False, True)), (1, 71, 131, 33, (False, True)),
        (1, big_h - 2, 233, 5, (False,)), (2, big_h, 233, 5, (False,)),
    ]
    for N, H, W, width, forms in sweep:
        m = blob_masks(rng, N, H, W, max(2, width // 2 + 1))
        inst = rng.uniform(30, 70, size=(N, H, W)).astype(np.float32)
        present = np.arange(N) % 2 == 0
        bw, isw = float(rng.uniform(1.1, 4.0)), float(rng.uniform(1.0, 3.0))
        want_w, want_d2 = O.weight_map(m, width, bw, isw, inst, present)
        for tiled in forms:
            w, d2 = raw_weight_map(dev(m), width, bw, isw, dev(inst), dev(present, torch.uint8), tiled=tiled)
            assert torch.equal(d2.cpu(), torch.from_numpy(want_d2)), (H, W, width, tiled)
            assert torch.equal(w.cpu(), torch.from_numpy(want_w)), (H, W, width, tiled)
        if H * W > 1000:
            continue
        x = (rng.standard_normal((N, 3, H, W)) * 2).astype(np.float32)
        cw = rng.uniform(0.5, 1.5, 3).astype(np.float32)
        for use_focal, gamma, cwv in ((False, 2.0, None), (False, 2.0, cw), (True, 2.0, cw), (True, 1.5, None)):
            vals, grad = O.loss(x, m, want_w, cwv, use_focal, gamma, 0.8, 1.25)
            out, dp = raw_loss(dev(x), dev(m), dev(want_w), None if cwv is None else dev(cwv), use_focal, gamma,
                               0.8, 1.25, gscale=0.5)
            got = out.cpu().tolist()
            for i, k in enumerate(("total_loss", "ce_loss", "dice_loss", "boundary_accuracy", "avg_boundary_weight")):
                assert got[i] == pytest.approx(vals[k], rel=1e-5, abs=1e-6 if k == "boundary_accuracy" else 0), k
            assert float((dp.cpu().double() - 0.5 * torch.from_numpy(grad)).abs().max()) <= 1e-5 * np.abs(0.5 * grad).max()
    # above the resident limit the halo-tiled form takes radii up to 32; a larger one is refused, not mis-computed
    m = dev(blob_masks(rng, 1, big_h, 233, 9))
    d2 = torch.empty(1, big_h, 233, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(L.lib().hiseg_distance_ws(1, big_h, 233)), dtype=torch.float32, device=DEV)
    assert L.lib().hiseg_distance_transform(m.data_ptr(), 1, big_h, 233, 40, 41 * 41, 0, d2.data_ptr(), ws.data_ptr(),
                                            L.stream_ptr()) == -2
    assert b"halo-tiled" in L.lib().hiseg_last_error_string()


def _case(G, adaptive):
    import hiseg
    cw = dev(G["factory_class_weights"])
    loss_fn = hiseg.DistanceAwareSegmentationLoss(class_weights=cw, use_focal=False)
    if adaptive:
        loss_fn = hiseg.AdaptiveBoundaryLoss(loss_fn).to(DEV)
        with torch.no_grad():
            loss_fn.boundary_weight.fill_(2.75)
    return loss_fn


def _run(loss_fn, x, t, inst):
    pred = x.clone().requires_grad_(True)
    total, d = loss_fn(pred, t, inst)
    total.backward()
    return total.detach().clone(), d._out.clone(), pred.grad.clone()


def test_two_runs_are_bit_identical(G):
    t, x, inst = dev(G["b_t"], torch.int64), dev(G["b_x"]), dev(G["b_straddle"])
    for adaptive in (False, True):
        a = _run(_case(G, adaptive), x, t, inst)
        b = _run(_case(G, adaptive), x, t, inst)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        assert torch.isfinite(a[2]).all()


@pytest.mark.parametrize("adaptive", [False, True])
def test_graph_capture_equals_eager(G, adaptive):
    """Forward and backward captured on one stream, replayed on new targets and logits: no host synchronisation
    (a capture fails on one), and the replay equals the eager result bit for bit."""
    t0, x0, inst0 = dev(G["b_t"], torch.int64), dev(G["b_x"]), dev(G["b_straddle"])
    t1 = torch.flip(t0, dims=(0, 2)).contiguous()
    x1 = (torch.flip(x0, dims=(0, 3)) * 0.5 + 0.1).contiguous()
    inst1 = (100.0 - inst0).contiguous()
    loss_fn = _case(G, adaptive)
    sx, st, si = x0.clone().requires_grad_(True), t0.clone(), inst0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):   # warm-up: the distance table and the class weights are uploaded once, here
            total, _ = loss_fn(sx, st, si)
            total.backward()
            sx.grad = None
        del total
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total, d = loss_fn(sx, st, si)
        total.backward()
    with torch.no_grad():
        sx.copy_(x1)
        st.copy_(t1)
        si.copy_(inst1)
    graph.replay()
    torch.cuda.synchronize()
    want = _run(loss_fn, x1, t1, inst1)
    assert torch.equal(total.detach(), want[0]) and torch.equal(d._out, want[1]) and torch.equal(sx.grad, want[2])
    first = _run(loss_fn, x0, t0, inst0)
    assert not torch.equal(first[0], want[0])   # the replay saw the new inputs, not the captured ones


def test_evaluate_model_passes_instance_info(G):
    """hiseg.metrics.evaluate_model hands the batch's 'instance_info' to the distance-aware losses."""
    import hiseg
    t, x, inst = dev(G["s_t"], torch.int64), dev(G["s_x"]), G["s_straddle"]

    class Fixed(nn.Module):
        def forward(self, images, rois):
            return x, {}

    info = [{"instance_distances": torch.from_numpy(inst[i])} for i in range(3)]
    batches = [{"image": torch.zeros(1), "roi_boxes": torch.zeros(1), "roi_masks": t.cpu(), "instance_info": info},
               {"image": torch.zeros(1), "roi_boxes": torch.zeros(1), "roi_masks": t.cpu()}]
    loss_fn = hiseg.DistanceAwareSegmentationLoss(boundary_width=3)
    m = hiseg.evaluate_model(Fixed(), batches, loss_fn, DEV)
    with_info, without = float(loss_fn(x, t, info)[0].detach()), float(loss_fn(x, t, None)[0].detach())
    assert with_info != without
    assert m["total_loss"] == pytest.approx((with_info + without) / 2, rel=1e-6)
    assert with_info == pytest.approx(float(G["s_inst_straddle_vals"][0]), rel=1e-5)


def test_train_step_of_the_b0_model_under_the_distance_loss(G):
    """One train step of the B0-std test model: finite loss, a finite gradient on every trainable parameter, and the
    step's d loss / d logits equal to the stand-alone loss backward on the same logits."""
    import hiseg
    from hiseg import train_engine as TE
    m = hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))
    filler.fill_module(m)
    for mod in m.modules():
        if isinstance(mod, (nn.Dropout, nn.Dropout2d)):
            mod.p = 0.0
    hiseg.set_compute_dtype(m, torch.float32)
    for mm in (m.roi_align_mask, m.roi_align_rgb):
        mm.spatial_scale_h, mm.spatial_scale_w = 96, 128
    m = m.to(DEV).train()
    images = dev(filler.uniform(61, (2, 3, 96, 128)))
    u = dev(filler.normal(62, (2, 1, 96, 128)) * 2.0)
    rois = torch.tensor([[0, .10, .10, .40, .90], [1, .35, .15, .80, .95], [0, .55, .05, .95, .70]]).to(DEV)
    tgt = dev(filler.ellipse_targets(63, 3, 128, 96))
    loss_fn = hiseg.create_distance_aware_loss({"background": 0.485, "target": 0.393, "non_target": 0.122},
                                               device=DEV)
    logits, _ = TE.train_forward(m, images, rois, u_override=u)
    logits.retain_grad()
    loss, d = loss_fn(logits, tgt)
    loss.backward()
    assert np.isfinite(float(loss)) and all(np.isfinite(v) for v in d.values())
    assert d["avg_boundary_weight"] > 1.0 and 0.0 <= d["boundary_accuracy"] <= 1.0
    # the distance decoder's threshold shapes only the auxiliary distance map, which this loss does not read: a loss
    # on the logits alone leaves it without a gradient (None in the reference's autograd as well); nothing else may
    missing = [n for n, p in m.named_parameters() if p.requires_grad and p.grad is None]
    assert set(missing) <= {"segmentation_head.distance_decoder.threshold"}, missing
    for n, p in m.named_parameters():
        if p.requires_grad and n not in missing:
            assert torch.isfinite(p.grad).all(), n
    alone = logits.detach().clone().requires_grad_(True)
    loss2, _ = loss_fn(alone, tgt)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(alone.grad, logits.grad)
