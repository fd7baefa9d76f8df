"""Full-frame instance composition on the GPU against the reference's own consumer (tests/golden/compose.npz,
gen_compose_golden.py): packed target masks, scores, the label map and the overlay; then the properties the serving
path relies on (front ends agree, ROI order, empty input, graph replay, the wrapper hook)."""
import numpy as np
import pytest
import torch

import filler
from helpers import b0_kwargs, hiseg_kwargs, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("tiny", "odd_12x10", "odd_10x12", "c2", "many")
_cache = {}


def case(name):
    """The fixture's arrays of one case on the device (loaded once, never modified)."""
    if name not in _cache:
        g = load("compose")
        c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
        d = {"logits": torch.from_numpy(c["logits"].astype(np.float32)).to(DEV),
             "rois": torch.from_numpy(c["rois"]).to(DEV), "frame": tuple(int(v) for v in c["frame"]),
             "image": torch.from_numpy(c["image"]).to(DEV), "colors": torch.from_numpy(c["colors"]).to(DEV)}
        _cache[name] = (c, d)
    return _cache[name]


def unpack(bits, mw):
    """int32 [N,mh,words] -> bool [N,mh,mw]; also checks that the padding bits are clear."""
    b = bits.cpu().numpy().view(np.uint32)
    N, mh, wpr = b.shape
    assert wpr == (mw + 31) // 32
    full = ((b[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(N, mh, wpr * 32).astype(bool)
    assert not full[..., mw:].any()
    return full[..., :mw]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tag,thr", (("", 0.5), ("_t0", 0.0)))
def test_classify_packs_the_reference_s_masks_and_scores(name, tag, thr):
    """Every bit and count equal; the score within 1e-5 absolute (scores lie in (0.5, 1]: an f32 mean of at most
    12 288 terms through a 256-lane tree is within about (48 + 8) * 2^-24 relative, expf differences add about 1e-6)."""
    from hiseg import ops
    c, d = case(name)
    bits, score, count = ops.roi_mask_classify(d["logits"], thr)
    mask = unpack(bits, d["logits"].shape[-1])
    want = c["mask" + tag].astype(bool)
    assert np.array_equal(mask, want)
    assert np.array_equal(count.cpu().numpy(), want.reshape(len(want), -1).sum(1))
    err = np.abs(score.cpu().numpy().astype(np.float64) - c["score" + tag].astype(np.float64)).max()
    print(f"{name}{tag}: score max abs err {err:.3e}")
    assert err <= 1e-5
    if thr == 0.0:      # the exact ties of the fixture: class 0 = class 1 on top is not a target, class 1 = class 2 is
        l = c["logits"].astype(np.float32)
        t01 = (l[:, 0] == l[:, 1]) & (l[:, 2] < l[:, 0])
        t12 = (l[:, 1] == l[:, 2]) & (l[:, 0] < l[:, 1])
        assert not mask[t01].any() and mask[t12].all()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tag,thr", (("", 0.5), ("_t0", 0.0)))
def test_label_map_is_the_reference_s(name, tag, thr):
    import hiseg
    c, d = case(name)
    label, score = hiseg.InstanceMapComposer(score_threshold=thr)(d["logits"], d["rois"], d["frame"])
    assert label.dtype == torch.int32 and tuple(label.shape) == d["frame"]
    assert np.array_equal(label.cpu().numpy(), c["label" + tag].astype(np.int32))
    assert tuple(score.shape) == (len(d["rois"]),)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("alpha", (0.5, 0.3))
def test_overlay_is_the_reference_s_at_every_byte(name, alpha):
    import hiseg
    c, d = case(name)
    comp = hiseg.InstanceMapComposer()
    label, _ = comp(d["logits"], d["rois"], d["frame"])
    out = comp.overlay(label, d["image"], d["colors"], alpha)
    assert out.dtype == torch.uint8 and out.shape == d["image"].shape
    assert np.array_equal(out.cpu().numpy(), c[f"overlay_a{int(alpha * 100)}"])


@pytest.mark.parametrize("name", CASES)
def test_pack_front_end_agrees_with_the_logits_front_end_at_threshold_zero(name):
    """instance_masks are the (argmax == 1) planes; with score_threshold 0 the logits front end sets the same pixels,
    and both scores are positive exactly where a pixel is set: the same label map, the fixture's."""
    import hiseg
    from hiseg import ops
    c, d = case(name)
    planes = ops.instance_masks(d["logits"])                             # the exported contract's own kernel
    assert np.array_equal(planes.cpu().numpy()[:, 0], c["mask_t0"].astype(np.float32))   # (np.argmax == 1)
    a, sa = hiseg.InstanceMapComposer(from_logits=False)(planes, d["rois"], d["frame"])
    b, sb = hiseg.InstanceMapComposer(score_threshold=0.0)(d["logits"], d["rois"], d["frame"])
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), c["label_t0"].astype(np.int32))
    assert torch.equal(sa, (sb > 0).float())
    bits_a, _, count_a = ops.roi_mask_pack(planes)
    bits_b, _, count_b = ops.roi_mask_classify(d["logits"], 0.0)
    assert torch.equal(bits_a, bits_b) and torch.equal(count_a, count_b)


def test_roi_order_decides_the_owner():
    import hiseg
    c, d = case("many")
    comp = hiseg.InstanceMapComposer()
    rev, _ = comp(d["logits"].flip(0), d["rois"].flip(0), d["frame"])
    assert np.array_equal(rev.cpu().numpy(), c["label_rev"].astype(np.int32))
    fwd, _ = comp(d["logits"], d["rois"], d["frame"])
    N = len(d["rois"])
    renamed = torch.where(fwd > 0, N + 1 - fwd, fwd)     # the same owners under the reversed numbering
    assert not torch.equal(rev, renamed)                  # the order, not only the numbering, changed the result
    assert torch.equal(rev > 0, fwd > 0)                  # while the painted area is the same


def test_no_rois_gives_an_empty_map():
    import hiseg
    from hiseg import ops
    logits = torch.zeros(0, 3, 12, 10, device=DEV)
    rois = torch.zeros(0, 5, device=DEV)
    label, score = hiseg.InstanceMapComposer()(logits, rois, (2, 37, 53))
    assert tuple(label.shape) == (2, 37, 53) and not label.any() and score.numel() == 0
    bits, score, count = ops.roi_mask_pack(torch.zeros(0, 1, 12, 10, device=DEV))
    assert tuple(bits.shape) == (0, 12, 1) and count.numel() == 0
    image = torch.full((2, 37, 53, 3), 201, dtype=torch.uint8, device=DEV)
    out = ops.instance_overlay(label, image, torch.zeros(0, 3, dtype=torch.uint8, device=DEV), 0.5)
    assert (out == 100).all()                             # 100.5 rounds half to even: dimmed, nothing painted
    assert ops.compose_instance_map(bits, score, rois, (0, 37, 53), 10).numel() == 0


def test_boxes_outside_the_frame_are_clipped():
    """Where the reference raises: the box is clipped to the frame, the mask still mapped over the unclipped box."""
    from hiseg import ops
    mh, mw, H, W = 4, 6, 10, 16
    masks = torch.zeros(1, 1, mh, mw, device=DEV)
    masks[0, 0, :, ::2] = 1                               # even source columns
    rois = torch.tensor([[0, -0.5, -0.25, 1.5, 1.125]], device=DEV)     # pixels [-8, -2, 24, 11]
    bits, score, _ = ops.roi_mask_pack(masks)
    label = ops.compose_instance_map(bits, score, rois, (1, H, W), mw).cpu().numpy()
    x1, y1, x2, y2 = -8, -2, 24, 11
    sx = np.minimum(np.floor((np.arange(W) - x1) * (1.0 / ((x2 - x1) / float(mw)))).astype(int), mw - 1)
    want = np.tile((sx % 2 == 0).astype(np.int32), (H, 1))[None]
    assert np.array_equal(label, want)
    nan = torch.tensor([[0, float("nan"), 0, 1, 1]], device=DEV)
    assert not ops.compose_instance_map(bits, score, nan, (1, H, W), mw).any()


def test_graph_replay_is_bit_identical_to_eager():
    import hiseg
    _, d = case("odd_10x12")
    comp = hiseg.InstanceMapComposer()

    def run():
        label, score = comp(d["logits"], d["rois"], d["frame"])
        return label, score, comp.overlay(label, d["image"], d["colors"], 0.3)

    eager = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                             # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for _ in range(3):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------- serving hook
def _serving():
    if "serving" not in _cache:
        import hiseg
        m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))).eval().to(DEV)
        hiseg.set_compute_dtype(m, torch.bfloat16)
        batches = []
        for k in range(3):
            images = torch.from_numpy(filler.uniform(500 + k, (2, 3, 96, 128))).to(DEV)
            rois = torch.from_numpy(filler.box_rois(600 + k, 2, 3)).to(DEV)
            batches.append((images, rois))
        _cache["serving"] = (m, batches)
    return _cache["serving"]


def _by_hand(inst, rois, frame):
    from hiseg import ops
    bits, score, _ = ops.roi_mask_pack(inst)
    return ops.compose_instance_map(bits, score, rois, frame, inst.shape[-1])


@pytest.mark.parametrize("frame_hw", (None, (37, 53)))
def test_wrapper_returns_the_instance_map_of_its_instance_masks(frame_hw):
    import hiseg
    m, batches = _serving()
    post = hiseg.BinaryMaskEdgeSmoothing().to(DEV)
    comp = hiseg.InstanceMapComposer(frame_size=frame_hw, from_logits=False)
    w = hiseg.RGBHierarchicalExportWrapper(m, instance_post=post, compose=comp)
    plain = hiseg.RGBHierarchicalExportWrapper(m, instance_post=post)
    painted = 0
    with torch.no_grad():
        for images, rois in batches:
            inst, binary, imap = w(images, rois)
            inst0, binary0 = plain(images, rois)
            assert torch.equal(inst, inst0) and torch.equal(binary, binary0)
            frame = (2, *(frame_hw or (96, 128)))
            assert imap.dtype == torch.int32 and tuple(imap.shape) == frame
            assert torch.equal(imap, _by_hand(inst, rois, frame))
            painted += int((imap > 0).sum())
    assert painted > 0


@pytest.mark.parametrize("gate", (False, True))
def test_stream_pipelined_export_composes_on_the_head_stream(gate):
    import hiseg
    m, batches = _serving()
    kw = dict(gate=True, gate_min_gflop=0.05) if gate else {}
    w = hiseg.RGBHierarchicalExportWrapper(m, compose=hiseg.InstanceMapComposer(from_logits=False))
    with torch.no_grad():
        serial = [w(i, r) for i, r in batches]
        piped = hiseg.StreamPipelinedExport(w, **kw).run(batches)
        none = hiseg.StreamPipelinedExport(hiseg.RGBHierarchicalExportWrapper(m), **kw).run(batches)
    torch.cuda.synchronize()
    assert len(piped) == len(none) == 3
    for s, p, n, (images, rois) in zip(serial, piped, none, batches):
        assert len(s) == len(p) == 3 and len(n) == 2
        for a, b in zip(s, p):
            assert torch.equal(a, b)
        assert torch.equal(p[2], _by_hand(p[0], rois, (2, 96, 128)))
        assert torch.equal(n[0], p[0]) and torch.equal(n[1], p[1])
