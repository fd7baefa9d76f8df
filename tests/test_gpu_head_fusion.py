"""The target branch's fused operands (round 7) against the separate passes they replace, bit for bit.

* ``conv2d(px_scale=att)``: the spatial-attention multiply inside the pointwise kernel's loader (conv_pw.hip PXS,
  the ConvTranspose 256 -> 4 x 128 form) == ops.pixel_scale followed by the same conv.
* ``conv2d(head2=...)``: the branch's last 1x1 (128 -> 2) in the epilogue of the 3x3 halo kernel (conv_hwc.hip H2)
  followed by the short hier_combine == the conv followed by the hier_combine that reads its whole output.
* End to end: engine.hier_head on the golden B0 head (bf16) == the same head with both fusions bypassed (the old ops
  calls).  Both fusions keep every bit, so the bar is equality -- tighter than any bf16 tolerance.

Shapes: pixel counts that are no multiple of the pointwise kernel's 32-pixel block with image boundaries inside a
block; ragged 16 x 16 pixel tiles and two tile columns / rows for the halo kernel.  Outputs start as NaN where a
buffer is passed in, so a form that writes nothing fails."""
import pytest
import torch
import torch.nn as nn

import filler
from helpers import b0_kwargs

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = torch.bfloat16


def _bn(c, g):
    bn = nn.BatchNorm2d(c).to(DEV).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, device=DEV, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(c, device=DEV, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
    return bn


# ------------------------------------------------------------------ fusion 1: per-pixel input scale
@pytest.mark.parametrize("H,W", [(10, 6), (16, 12)])
def test_px_scale_in_conv_transpose_loader_equals_pixel_scale_pass(H, W):
    from hiseg import ops
    N, Ca, C = 3, 256, 128
    g = torch.Generator(device=DEV).manual_seed(11)
    x = ops.Act.from_nchw(torch.randn(N, Ca, H, W, device=DEV, generator=g), DT)
    att = torch.rand(N * H * W, device=DEV, generator=g)   # a sigmoid's range
    w = torch.randn(Ca, C, 2, 2, device=DEV, generator=g) / Ca ** 0.5
    p = ops.pack_convT2x2(w, torch.randn(C, device=DEV, generator=g) * 0.1, _bn(C, g), 1, DT, DEV)
    assert p.gemm_cols == 512
    assert ops._fused_ok(p, x, None, None, None, None, att, None, DT, 1), "the ConvTranspose form must be fused"
    ref = ops.conv2d(p, ops.pixel_scale(x, att))
    got = ops.conv2d(p, x, px_scale=att)
    torch.cuda.synchronize()
    assert (got.N, got.H, got.W, got.C) == (N, 2 * H, 2 * W, C)
    assert torch.isfinite(got.t.float()).all()
    assert torch.equal(got.t, ref.t)
    # the scale matters (the comparison above is not of two unscaled convs)
    assert not torch.equal(got.t, ops.conv2d(p, x).t)


def test_px_scale_falls_back_where_the_layer_has_no_fused_form():
    """A plain 1x1 layer (no ConvTranspose) and f32: conv2d runs the pixel_scale pass itself, same result."""
    from hiseg import ops
    N, H, W, Ca, C = 2, 7, 5, 64, 64
    g = torch.Generator(device=DEV).manual_seed(12)
    att = torch.rand(N * H * W, device=DEV, generator=g)
    w = torch.randn(C, Ca, 1, 1, device=DEV, generator=g) / Ca ** 0.5
    xin = torch.randn(N, Ca, H, W, device=DEV, generator=g)
    for dt in (DT, torch.float32):
        x = ops.Act.from_nchw(xin, dt)
        p = ops.pack_conv(w, None, None, 1, dt, DEV)
        assert not ops._fused_ok(p, x, None, None, None, None, att, None, dt, 1)
        assert torch.equal(ops.conv2d(p, x, px_scale=att).t, ops.conv2d(p, ops.pixel_scale(x, att)).t)


def test_attn_map_and_pixel_scale_are_the_halves_of_attn_spatial():
    from hiseg import ops
    N, H, W, C = 2, 9, 7, 64
    g = torch.Generator(device=DEV).manual_seed(13)
    x = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT)
    w7 = torch.randn(1, 2, 7, 7, device=DEV, generator=g) * 0.1
    assert torch.equal(ops.pixel_scale(x, ops.attn_map(x, w7)).t, ops.attn_spatial(x, w7).t)


# ------------------------------------------------------------------ fusion 3: the last 1x1 in conv2's epilogue
def _combine_args(N, h, w, g):
    low = torch.randn(N * h * w * 2, device=DEV, generator=g)
    ut_w = torch.randn(2, 32, 2, 2, device=DEV, generator=g) * 0.3
    ut_s = torch.rand(32, device=DEV, generator=g) + 0.5
    ut_h = torch.randn(32, device=DEV, generator=g) * 0.1
    u1_w = torch.randn(2, 32, device=DEV, generator=g) * 0.2
    u1_b = torch.randn(2, device=DEV, generator=g) * 0.1
    return low, ut_w, ut_s, ut_h, u1_w, u1_b


@pytest.mark.parametrize("want_aux", [False, True])
@pytest.mark.parametrize("H,W", [(24, 32), (32, 24)])
def test_head2_epilogue_and_short_combine_equal_conv_then_combine(H, W, want_aux):
    from hiseg import ops
    N, C = 3, 128
    g = torch.Generator(device=DEV).manual_seed(21)
    x = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT)
    res = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT)
    w = torch.randn(C, C, 3, 3, device=DEV, generator=g) / (9 * C) ** 0.5
    p = ops.pack_conv(w, None, _bn(C, g), 1, DT, DEV, pad=1)
    t_w = (torch.randn(2, C, device=DEV, generator=g) / C ** 0.5).contiguous()
    t_b = torch.randn(2, device=DEV, generator=g) * 0.1
    low, ut_w, ut_s, ut_h, u1_w, u1_b = _combine_args(N, H // 2, W // 2, g)

    t = ops.conv2d(p, x, residual=res)
    ref = ops.hier_combine(low, N, H // 2, W // 2, t, ut_w, ut_s, ut_h, 1, u1_w, u1_b, t_w, t_b, want_aux)

    h2 = ops.Head2(t_w, t_b)
    assert ops.conv2d(p, x, residual=res, head2=h2) is None, "the 128 -> 128 residual form must be fused"
    assert h2.out is not None and tuple(h2.out.shape) == (N * H * W, 2)
    got = ops.hier_combine(low, N, H // 2, W // 2, None, ut_w, ut_s, ut_h, 1, u1_w, u1_b, t_w, t_b, want_aux,
                           tn2=h2.out)
    torch.cuda.synchronize()
    assert torch.isfinite(h2.out).all()
    assert torch.equal(got[0], ref[0])
    if want_aux:
        assert torch.equal(got[1], ref[1])
        assert torch.equal(got[2], ref[2])
        # tn is the 1x1 itself: the epilogue's two numbers per pixel, NCHW
        assert torch.equal(got[2], h2.out.view(N, H, W, 2).permute(0, 3, 1, 2))
    else:
        assert got[1] is None and got[2] is None


def test_head2_falls_back_where_the_layer_has_no_fused_form():
    """64 output channels (the workgroup tile is 64-Cout x 16 x 32 pixels) and a layer without a residual: conv2d
    runs the layer as usual, returns its output and leaves Head2.out None."""
    from hiseg import ops
    N, H, W = 2, 16, 16
    g = torch.Generator(device=DEV).manual_seed(22)
    for C, with_res in ((64, True), (128, False)):
        x = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT)
        res = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT) if with_res else None
        p = ops.pack_conv(torch.randn(C, C, 3, 3, device=DEV, generator=g) / (9 * C) ** 0.5, None, None, 1, DT, DEV,
                          pad=1)
        h2 = ops.Head2(torch.randn(2, C, device=DEV, generator=g), torch.zeros(2, device=DEV))
        out = ops.conv2d(p, x, residual=res, head2=h2)
        assert out is not None and h2.out is None
        assert torch.equal(out.t, ops.conv2d(p, x, residual=res).t)


# ------------------------------------------------------------------ end to end: the golden B0 head, bf16
def test_hier_head_equals_the_head_with_both_fusions_bypassed(monkeypatch):
    import hiseg
    from hiseg import engine, ops
    from hiseg.layers import RefinedHierarchicalSegmentationHead
    kw = b0_kwargs()
    head = filler.fill_module(RefinedHierarchicalSegmentationHead(
        256, 256, 3, tuple(kw["mask_size"]), use_attention_module=True, use_contour_detection=True,
        use_distance_transform=True, normalization_type="batchnorm", activation_function="relu",
        hierarchical_base_channels=kw["hierarchical_base_channels"],
        hierarchical_depth=kw["hierarchical_depth"])).eval().to(DEV)
    hiseg.set_compute_dtype(head, DT)
    x = torch.from_numpy(filler.normal(31, (2, 256, 64, 48))).to(DEV)   # tests/test_gpu_parity.py's head input

    fused = {"px_scale": 0, "head2": 0}
    real = ops.conv2d

    def counting(p, xa, *a, **k):
        out = real(p, xa, *a, **k)
        if k.get("px_scale") is not None:
            fused["px_scale"] += 1
        if k.get("head2") is not None and k["head2"].out is not None:
            fused["head2"] += 1
        return out

    real_ps = ops.pixel_scale

    def no_pixel_scale(*a, **k):
        fused["pixel_scale_pass"] = fused.get("pixel_scale_pass", 0) + 1
        return real_ps(*a, **k)

    monkeypatch.setattr(ops, "conv2d", counting)
    monkeypatch.setattr(ops, "pixel_scale", no_pixel_scale)
    new = {aux: engine.head_nchw(head, x) if aux == "full" else
           engine.hier_head(engine.Ctx(head, DT, x.device), head, ops.Act.from_nchw(x, DT), "none")
           for aux in ("full", "none")}
    assert fused == {"px_scale": 2, "head2": 2}, fused

    def bypass(p, xa, *a, px_scale=None, head2=None, **k):   # the launches of the parent commit
        if px_scale is not None:
            xa = ops.pixel_scale(xa, px_scale)
        return real(p, xa, *a, **k)

    monkeypatch.setattr(ops, "pixel_scale", real_ps)
    monkeypatch.setattr(ops, "conv2d", bypass)
    old_logits, old_aux = engine.head_nchw(head, x)
    old_none, _ = engine.hier_head(engine.Ctx(head, DT, x.device), head, ops.Act.from_nchw(x, DT), "none")
    torch.cuda.synchronize()
    logits, aux = new["full"]
    assert torch.isfinite(logits).all()
    assert torch.equal(aux["bg_fg_logits"], old_aux["bg_fg_logits"])
    assert torch.equal(aux["bg_fg_logits_low"], old_aux["bg_fg_logits_low"])
    assert torch.equal(aux["target_nontarget_logits"], old_aux["target_nontarget_logits"])
    assert torch.equal(logits, old_logits)
    assert torch.equal(new["none"][0], old_none)
