"""The target branch's channel gate (round 8) applied inside the two convs that read the gated tensor, against the
channel_scale pass it replaces, bit for bit.

* ``conv2d(a_gate=g)``: source A read as bf16(x * g[image][channel]) by the 3x3 halo kernel's loader (conv_hwc.hip GA:
  the halo pieces through registers) == ops.channel_scale followed by the same conv.
* ``conv2d(residual=x, res_gate=g, head2=...)``: the residual read as bf16(x * g[image][channel]) in the epilogue that
  also applies the trailing 1x1 (conv_hwc.hip H2 + RG) == the same conv on the channel_scale'd residual.
* Batch chunking: a batch whose operands exceed 2 GiB is split into image ranges (conv_dispatch.cpp); the gate tables
  must move with the images.
* Fallback: f32 and a 64-channel layer have no such form; conv2d runs the channel_scale pass itself.
* End to end: engine.hier_head on the golden B0 head (bf16) with the gate fused == the same head with the fusion
  bypassed, and the fused path runs no channel_scale.

Every product is rounded exactly as channel_scale_kernel rounds it, so the bar is equality of the stored bits.
Shapes: 24 x 40 and 40 x 24 give ragged 16 x 16 pixel tiles, two or more tile rows and columns, and 128 channels are
four 32-channel slices, so the ring of three halo buffers wraps.  Output buffers start as NaN where one is passed."""
import pytest
import torch
import torch.nn as nn

import filler
from helpers import b0_kwargs

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = torch.bfloat16
SHAPES = [(24, 40), (40, 24)]


def _bn(c, g):
    bn = nn.BatchNorm2d(c).to(DEV).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, device=DEV, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(c, device=DEV, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
    return bn


def _gate(N, C, g):
    """A sigmoid's range, different per image, one entry exactly 0 and one exactly 1."""
    gate = torch.rand(N, C, device=DEV, generator=g)
    gate[0, 5] = 0.0
    gate[N - 1, C - 3] = 1.0
    return gate.contiguous()


def _nan_out(N, H, W, C):
    from hiseg import ops
    out = ops.Act.new(N, H, W, C, DT, DEV, zero=False)
    out.t.fill_(float("nan"))
    return out


def _conv3x3(C, g, dt=DT):
    from hiseg import ops
    w = torch.randn(C, C, 3, 3, device=DEV, generator=g) / (9 * C) ** 0.5
    return ops.pack_conv(w, None, _bn(C, g), 1, dt, DEV, pad=1)


# ------------------------------------------------------------------ gated source A
@pytest.mark.parametrize("H,W", SHAPES)
def test_a_gate_in_halo_loader_equals_channel_scale_pass(H, W):
    from hiseg import ops
    N, C = 3, 128
    g = torch.Generator(device=DEV).manual_seed(41)
    x = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT)
    gate = _gate(N, C, g)
    p = _conv3x3(C, g)
    assert ops._fused_ok(p, x, None, None, None, None, None, None, DT, 1, a_gate=gate), \
        "the 128 -> 128 ReLU form must be fused"
    ref = ops.conv2d(p, ops.channel_scale(x, gate), out=_nan_out(N, H, W, C))
    got = ops.conv2d(p, x, a_gate=gate, out=_nan_out(N, H, W, C))
    plain = ops.conv2d(p, x)
    perm = ops.conv2d(p, x, a_gate=gate[[1, 2, 0]].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(got.t.float()).all()
    assert torch.equal(got.t, ref.t)
    assert not torch.equal(got.t, plain.t), "the gate must matter"
    assert not torch.equal(got.t, perm.t), "each image must read its own row of the gate"
    for n in range(N):   # (and every image differs from its permuted-gate result, not just one of them)
        a, b = got.t.view(N, -1)[n], perm.t.view(N, -1)[n]
        assert not torch.equal(a, b)


# ------------------------------------------------------------------ gated residual beside the trailing 1x1
def _combine_args(N, h, w, g):
    low = torch.randn(N * h * w * 2, device=DEV, generator=g)
    ut_w = torch.randn(2, 32, 2, 2, device=DEV, generator=g) * 0.3
    ut_s = torch.rand(32, device=DEV, generator=g) + 0.5
    ut_h = torch.randn(32, device=DEV, generator=g) * 0.1
    u1_w = torch.randn(2, 32, device=DEV, generator=g) * 0.2
    u1_b = torch.randn(2, device=DEV, generator=g) * 0.1
    return low, ut_w, ut_s, ut_h, u1_w, u1_b


@pytest.mark.parametrize("want_aux", [False, True])
@pytest.mark.parametrize("H,W", SHAPES)
def test_res_gate_with_head2_equals_channel_scaled_residual(H, W, want_aux):
    from hiseg import ops
    N, C = 3, 128
    g = torch.Generator(device=DEV).manual_seed(42)
    h = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT)
    x = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), DT)
    gate = _gate(N, C, g)
    p = _conv3x3(C, g)
    t_w = (torch.randn(2, C, device=DEV, generator=g) / C ** 0.5).contiguous()
    t_b = torch.randn(2, device=DEV, generator=g) * 0.1
    low, ut_w, ut_s, ut_h, u1_w, u1_b = _combine_args(N, H // 2, W // 2, g)

    def combine(h2):
        return ops.hier_combine(low, N, H // 2, W // 2, None, ut_w, ut_s, ut_h, 1, u1_w, u1_b, t_w, t_b, want_aux,
                                tn2=h2.out)

    h2r = ops.Head2(t_w, t_b)
    assert ops.conv2d(p, h, residual=ops.channel_scale(x, gate), head2=h2r) is None
    ref = combine(h2r)
    h2g = ops.Head2(t_w, t_b)
    assert ops._fused_ok(p, h, None, x, None, None, None, h2g, DT, 1, res_gate=gate), "the H2 form must take the gate"
    assert ops.conv2d(p, h, residual=x, res_gate=gate, head2=h2g) is None
    got = combine(h2g)
    h2p = ops.Head2(t_w, t_b)
    assert ops.conv2d(p, h, residual=x, head2=h2p) is None
    h2q = ops.Head2(t_w, t_b)
    assert ops.conv2d(p, h, residual=x, res_gate=gate[[1, 2, 0]].contiguous(), head2=h2q) is None
    torch.cuda.synchronize()
    assert torch.isfinite(h2g.out).all()
    assert torch.equal(h2g.out, h2r.out)
    assert not torch.equal(h2g.out, h2p.out), "the gate must matter"
    assert not torch.equal(h2g.out, h2q.out), "each image must read its own row of the gate"
    assert torch.equal(got[0], ref[0])
    if want_aux:
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    else:
        assert got[1] is None and got[2] is None


# ------------------------------------------------------------------ batch chunking
def test_gate_tables_follow_the_image_ranges_of_a_split_batch():
    """hiseg_conv2d_fwd splits a batch whose largest operand exceeds 2 GiB - 1 MiB into ranges of
    floor((2 GiB - 1 MiB) / bytes per image) images.  16 x 16 x 128 bf16 images are 64 KiB: ranges of 32752 images, so
    32760 images run as 32752 + 8.  Every image holds the same pixels and only the gate rows differ, so a range that
    read the table from its start again would show in the last 8 images."""
    from hiseg import ops
    H = W = 16
    C = 128
    per = H * W * C * 2
    step = ((1 << 31) - (1 << 20)) // per
    N = step + 8
    assert N * per > (1 << 31) - (1 << 20) and step < N
    g = torch.Generator(device=DEV).manual_seed(43)
    img = torch.randn(H * W * C, device=DEV, generator=g).to(DT)
    x = ops.Act.new(N, H, W, C, DT, DEV, zero=False)
    x.t.view(N, -1).copy_(img[None].expand(N, -1))
    gate = _gate(N, C, g)
    p = _conv3x3(C, g)
    xs = ops.channel_scale(x, gate)
    ref = ops.conv2d(p, xs)
    got = ops.conv2d(p, x, a_gate=gate, out=_nan_out(N, H, W, C))
    torch.cuda.synchronize()
    assert torch.equal(got.t, ref.t)
    assert not torch.equal(got.t.view(N, -1)[step:], got.t.view(N, -1)[:8])   # (the tail has gates of its own)

    t_w = (torch.randn(2, C, device=DEV, generator=g) / C ** 0.5).contiguous()
    t_b = torch.randn(2, device=DEV, generator=g) * 0.1
    h2r, h2g = ops.Head2(t_w, t_b), ops.Head2(t_w, t_b)
    assert ops.conv2d(p, ref, residual=xs, head2=h2r) is None
    del xs
    assert ops.conv2d(p, ref, residual=x, res_gate=gate, head2=h2g) is None
    torch.cuda.synchronize()
    assert torch.isfinite(h2g.out).all()
    assert torch.equal(h2g.out, h2r.out)


# ------------------------------------------------------------------ fallback
def test_gates_fall_back_where_the_layer_has_no_fused_form():
    """f32, and a 64-channel layer (64-Cout x 16 x 32-pixel tiles): conv2d runs the channel_scale pass itself."""
    from hiseg import ops
    N, H, W = 2, 16, 16
    g = torch.Generator(device=DEV).manual_seed(44)
    for C, dt in ((128, torch.float32), (64, DT)):
        xin = torch.randn(N, C, H, W, device=DEV, generator=g)
        x = ops.Act.from_nchw(xin, dt)
        h = ops.Act.from_nchw(torch.randn(N, C, H, W, device=DEV, generator=g), dt)
        gate = _gate(N, C, g)
        p = _conv3x3(C, g, dt)
        assert not ops._fused_ok(p, x, None, None, None, None, None, None, dt, 1, a_gate=gate)
        got = ops.conv2d(p, x, a_gate=gate)
        ref = ops.conv2d(p, ops.channel_scale(x, gate))
        assert torch.equal(got.t, ref.t)
        assert not torch.equal(got.t, ops.conv2d(p, x).t)
        # the residual's gate without / with a trailing 1x1 the layer cannot fuse either
        got = ops.conv2d(p, h, residual=x, res_gate=gate)
        ref = ops.conv2d(p, h, residual=ops.channel_scale(x, gate))
        assert torch.equal(got.t, ref.t)
        h2 = ops.Head2(torch.randn(2, C, device=DEV, generator=g), torch.zeros(2, device=DEV))
        if dt == DT:
            got = ops.conv2d(p, h, residual=x, res_gate=gate, head2=h2)
            assert got is not None and h2.out is None and torch.equal(got.t, ref.t)


# ------------------------------------------------------------------ end to end: the golden B0 head, bf16
def test_hier_head_equals_the_head_with_the_gate_fusion_bypassed(monkeypatch):
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
    x = torch.from_numpy(filler.normal(31, (2, 256, 64, 48))).to(DEV)   # tests/test_gpu_head_fusion.py's head input

    calls = {"channel_scale": 0, "a_gate": 0, "res_gate": 0}
    real_conv, real_cs, real_ok = ops.conv2d, ops.channel_scale, engine.gated_block_ok

    def counting_conv(p, xa, *a, **k):
        calls["a_gate"] += k.get("a_gate") is not None
        calls["res_gate"] += k.get("res_gate") is not None
        return real_conv(p, xa, *a, **k)

    def counting_cs(*a, **k):
        calls["channel_scale"] += 1
        return real_cs(*a, **k)

    def run():
        full = engine.head_nchw(head, x)
        none = engine.hier_head(engine.Ctx(head, DT, x.device), head, ops.Act.from_nchw(x, DT), "none")
        torch.cuda.synchronize()
        return full, none

    monkeypatch.setattr(ops, "conv2d", counting_conv)
    monkeypatch.setattr(ops, "channel_scale", counting_cs)
    (logits, aux), (logits_none, _) = run()
    assert calls == {"channel_scale": 0, "a_gate": 2, "res_gate": 2}, calls

    monkeypatch.setattr(engine, "gated_block_ok", lambda *a, **k: False)   # the launches of the parent commit
    (old_logits, old_aux), (old_none, _) = run()
    assert calls == {"channel_scale": 2, "a_gate": 2, "res_gate": 2}, calls
    monkeypatch.setattr(engine, "gated_block_ok", real_ok)
    assert torch.isfinite(logits).all()
    assert torch.equal(aux["bg_fg_logits"], old_aux["bg_fg_logits"])
    assert torch.equal(aux["target_nontarget_logits"], old_aux["target_nontarget_logits"])
    assert torch.equal(logits, old_logits)
    assert torch.equal(logits_none, old_none)
